"""CPU: point-to-plane ICP without a GPU — the fp64 restatement (tests/icp_plane_restatement.py) on a planted motion and on a coplanar
target, and the host-side domain checks of lcr_icp_plane_ws_bytes / lcr_icp_point_to_plane."""
import ctypes
import os

import numpy as np

import icp_plane_restatement as ipr
import icp_restatement as ir
import normals_restatement as nr
from conftest import GOLDEN

EARG, ESPACE = -1, -2


def test_restatement_recovers_planted_motion():
    from lcrnet_amd import evaluation as ev
    tgt = np.load(os.path.join(GOLDEN, "scans", "000026.npy"))
    nrm = nr.estimate_normals(tgt, 1.0, 30)["normals"].astype(np.float32)
    motion = ir.rigid([0.1, -0.2, 1.0], 3.0, [0.5, -0.3, 0.1])
    src = ir.planted_scan_pair(tgt, motion, seed=1)
    init = motion @ np.linalg.inv(ir.rigid([0, 0, 1], 1.0, [0.2, -0.15, 0.05]))
    r = ipr.icp(src, tgt, nrm, 0.5, init, max_iteration=100)
    rre, rte = ev.compute_registration_error(motion, r["T"])[:2]
    assert rre < 0.05 and rte < 0.005, (rre, rte)
    assert r["fitness"] > 0.9 and 0 < r["iterations"] < 100
    f, e = r["fitness_hist"], r["rmse_hist"]
    stops = [abs(f[k + 1] - f[k]) < 1e-6 and abs(e[k + 1] - e[k]) < 1e-6 for k in range(len(f) - 1)]
    assert stops[-1] and not any(stops[:-1])


def test_transform_vector6_matches_open3d_convention():
    x = np.array([0.01, -0.02, 0.03, 0.4, 0.5, -0.6])
    T = ipr.transform_vector6(x)
    ca, sa, cb, sb, cc, sc = np.cos(0.01), np.sin(0.01), np.cos(-0.02), np.sin(-0.02), np.cos(0.03), np.sin(0.03)
    R = np.array([[cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa], [sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa],
                  [-sb, cb * sa, cb * ca]])
    assert np.abs(T[:3, :3] - R).max() < 1e-15 and np.array_equal(T[:3, 3], x[3:])


def test_restatement_keeps_T_on_degenerate_targets():
    g = np.random.default_rng(0).uniform(-5, 5, (2000, 2))
    flat = np.stack([g[:, 0], g[:, 1], np.zeros(2000)], 1).astype(np.float32)
    up = np.tile(np.array([[0, 0, 1]], np.float32), (2000, 1))
    src = flat[:800] + np.float32(0.05)
    T0 = ir.rigid([0, 0, 1], 1.0, [0.1, 0, 0])
    corr = ir.correspondence_step(src, flat, T0, 0.5)["corr"]
    T, applied = ipr.plane_update(src, flat, up, corr, T0)               # one plane: A has rank 3
    assert not applied and np.array_equal(T, T0)
    T, applied = ipr.plane_update(src, flat, np.zeros_like(up), corr, T0)    # no normals: nothing usable
    assert not applied and np.array_equal(T, T0)


def test_ws_bytes_and_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    nb, pp = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert L.lcr_icp_plane_ws_bytes(16, 16 * 84000, 16 * 120000, ctypes.byref(nb)) == 0
    assert L.lcr_icp_ws_bytes(16, 16 * 84000, 16 * 120000, ctypes.byref(pp)) == 0
    assert nb.value >= pp.value + (16 * 84000 // 256) * 13 * 8                 # 30 doubles per block row against 17
    for args in ((0, 10, 10), (65, 10, 10), (1, -1, 10), (1, 10, -1), (1, 2**31, 10), (1, 10, 2**31)):
        assert L.lcr_icp_plane_ws_bytes(*args, ctypes.byref(nb)) == EARG, args
        assert b"lcr_icp_plane_ws_bytes" in L.lcr_last_error()

    fake = ctypes.c_void_p(256)

    def call(S=1, lens=(10,), tl=(10,), r=0.5, it=30, ce=16, nrm=fake, init=fake, ws_bytes=1 << 40):
        sl = np.asarray(list(lens) + [0] * 64, np.int64)
        tt = np.asarray(list(tl) + [0] * 64, np.int64)
        return L.lcr_icp_point_to_plane(fake, sl.ctypes.data, fake, tt.ctypes.data, nrm, S, init, r, it, 1e-6, 1e-6, fake, fake, fake, fake, None,
                                        None, None, None, ce, fake, ws_bytes, None)

    for kw in (dict(S=0), dict(S=65), dict(it=-1), dict(it=100_001), dict(r=0.0), dict(r=float("nan")), dict(r=1e20), dict(ce=-1),
               dict(lens=(-1,)), dict(tl=(-5,)), dict(nrm=None), dict(init=None)):
        assert call(**kw) == EARG, kw
        assert b"lcr_icp_point_to_plane" in L.lcr_last_error()
    assert call(ws_bytes=16) == ESPACE
