"""CPU: the point-to-point ICP without a GPU — the fp64 restatement (tests/icp_restatement.py) on a planted motion, and the host-side
domain checks of lcr_icp_ws_bytes / lcr_icp_point_to_point (refused before anything is launched)."""
import ctypes
import os

import numpy as np

import icp_restatement as ir
from conftest import GOLDEN

EARG, ESPACE = -1, -2


def test_restatement_recovers_planted_motion():
    from lcrnet_amd import evaluation as ev
    tgt = np.load(os.path.join(GOLDEN, "scans", "000026.npy"))
    motion = ir.rigid([0.1, -0.2, 1.0], 3.0, [0.5, -0.3, 0.1])
    src = ir.planted_scan_pair(tgt, motion, seed=1)
    init = motion @ np.linalg.inv(ir.rigid([0, 0, 1], 1.0, [0.2, -0.15, 0.05]))
    r = ir.icp(src, tgt, 0.5, init, max_iteration=100)
    rre, rte = ev.compute_registration_error(motion, r["T"])[:2]
    assert rre < 0.05 and rte < 0.005, (rre, rte)
    assert r["fitness"] > 0.9 and 0 < r["iterations"] < 100
    assert len(r["T_hist"]) == r["iterations"] + 1 and r["fitness_hist"][-1] == r["fitness"]
    # the stopping rule held at the last step and at no earlier one
    f, e = r["fitness_hist"], r["rmse_hist"]
    stops = [abs(f[k + 1] - f[k]) < 1e-6 and abs(e[k + 1] - e[k]) < 1e-6 for k in range(len(f) - 1)]
    assert stops[-1] and not any(stops[:-1])


def test_restatement_edge_cases():
    pts = np.random.default_rng(0).uniform(-5, 5, (200, 3)).astype(np.float32)
    empty = np.zeros((0, 3), np.float32)
    T0 = ir.rigid([0, 0, 1], 10.0, [1, 2, 3])
    for s, t in ((empty, pts), (pts, empty)):
        r = ir.icp(s, t, 0.5, T0)
        assert np.array_equal(r["T"], T0) and r["fitness"] == 0 and r["rmse"] == 0 and r["iterations"] == 0
    far = ir.icp(pts + np.float32(100), pts, 0.5, np.eye(4))              # nobody within r: T kept, converged after one update
    assert far["iterations"] == 1 and np.array_equal(far["T"], np.eye(4)) and far["fitness"] == 0 and (far["corr"] == -1).all()
    zero = ir.icp(pts, pts, 0.5, T0, max_iteration=0)
    assert zero["iterations"] == 0 and np.array_equal(zero["T"], T0) and len(zero["T_hist"]) == 1


def test_ws_bytes_and_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    assert L.lcr_icp_ws_bytes(16, 16 * 84000, 16 * 120000, ctypes.byref(nb)) == 0
    grid = ctypes.c_size_t(0)
    assert L.lcr_support_grid_ws_bytes(16 * 120000, 16, ctypes.byref(grid)) == 0
    assert nb.value >= grid.value + (16 * 84000 // 256) * 17 * 8
    for args in ((0, 10, 10), (65, 10, 10), (1, -1, 10), (1, 10, -1), (1, 2**31, 10), (1, 10, 2**31)):
        assert L.lcr_icp_ws_bytes(*args, ctypes.byref(nb)) == EARG, args
        assert b"lcr_icp_ws_bytes" in L.lcr_last_error()
    assert L.lcr_icp_ws_bytes(1, 10, 10, None) == EARG

    fake = ctypes.c_void_p(256)                                        # never dereferenced: the checks come first

    def call(S=1, lens=(10,), tl=(10,), r=0.5, it=30, rf=1e-6, rr=1e-6, ce=16, src=fake, init=fake, ws_bytes=1 << 40):
        sl = np.asarray(list(lens) + [0] * 64, np.int64)
        tt = np.asarray(list(tl) + [0] * 64, np.int64)
        return L.lcr_icp_point_to_point(src, sl.ctypes.data, fake, tt.ctypes.data, S, init, r, it, rf, rr, fake, fake, fake, fake, None, None, None,
                                        None, ce, fake, ws_bytes, None)

    for kw in (dict(S=0), dict(S=65), dict(it=-1), dict(it=100_001), dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")),
               dict(r=1e20), dict(ce=-1), dict(rf=-1e-6), dict(rr=float("nan")), dict(lens=(-1,)), dict(tl=(-5,)), dict(lens=(2**31,)),
               dict(src=None), dict(init=None)):
        assert call(**kw) == EARG, kw
        assert b"lcr_icp_point_to_point" in L.lcr_last_error()
    assert call(ws_bytes=16) == ESPACE
