"""CPU: surface normals without a GPU — the fp64 restatement (tests/normals_restatement.py) on noise-free planes, and the host-side domain
checks of lcr_normals_ws_bytes / lcr_estimate_normals (refused before anything is launched)."""
import ctypes

import numpy as np

import normals_restatement as nr

EARG, ESPACE = -1, -2


def test_restatement_recovers_analytic_plane_normals():
    pts, normal, _ = nr.planes_cloud(3000, seed=1)
    out = nr.estimate_normals(pts, 0.9, 30)
    assert not out["degenerate"].any()
    cosang = (out["normals"] * normal).sum(axis=1)                     # oriented toward the origin, like the analytic normals
    assert cosang.min() > 1 - 1e-9, cosang.min()
    assert (out["count"] == 30).mean() > 0.9 and out["count"].max() == 30
    assert np.abs(out["curvature"]).max() < 1e-9


def test_restatement_degenerate_and_orientation_rules():
    line = np.stack([np.linspace(0, 1, 20), np.zeros(20), np.zeros(20)], 1).astype(np.float32)
    dup = np.tile(np.array([[1.0, 2.0, 3.0]], np.float32), (10, 1))
    for cloud in (line, dup, line[:2]):
        o = nr.estimate_normals(cloud, 0.5, 30)
        assert o["degenerate"].all() and not o["normals"].any() and not o["curvature"].any()
    g = np.random.default_rng(0).uniform(-1, 1, (500, 2))
    ground = np.stack([g[:, 0], g[:, 1], np.full(500, -1.0)], 1).astype(np.float32)
    up = nr.estimate_normals(ground, 0.5, 30)                            # sensor above the ground: normals point up
    assert (up["normals"][:, 2] > 0.999).all()
    down = nr.estimate_normals(ground, 0.5, 30, viewpoint=(0, 0, -5))
    assert (down["normals"][:, 2] < -0.999).all()
    one = nr.estimate_normals(ground, 0.5, 1)
    assert (one["count"] == 1).all() and one["degenerate"].all()


def test_ws_bytes_and_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    nb = ctypes.c_size_t(0)
    assert L.lcr_normals_ws_bytes(16, 16 * 120000, ctypes.byref(nb)) == 0
    grid = ctypes.c_size_t(0)
    assert L.lcr_support_grid_ws_bytes(16 * 120000, 16, ctypes.byref(grid)) == 0
    assert nb.value >= grid.value + 16 * 120000 * (6 * 8 + 4)
    for args in ((0, 10), (65, 10), (1, -1), (1, 2**31)):
        assert L.lcr_normals_ws_bytes(*args, ctypes.byref(nb)) == EARG, args
        assert b"lcr_normals_ws_bytes" in L.lcr_last_error()
    assert L.lcr_normals_ws_bytes(1, 10, None) == EARG

    fake = ctypes.c_void_p(256)                                        # never dereferenced: the checks come first

    def call(B=1, lens=(10,), r=0.5, nn=30, pts=fake, out=fake, ws=fake, ws_bytes=1 << 40):
        ln = np.asarray(list(lens) + [0] * 64, np.int64)
        return L.lcr_estimate_normals(pts, ln.ctypes.data, B, r, nn, None, out, None, None, ws, ws_bytes, None)

    for kw in (dict(B=0), dict(B=65), dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")), dict(r=1e20), dict(nn=0),
               dict(nn=129), dict(lens=(-1,)), dict(lens=(2**31,)), dict(pts=None), dict(out=None), dict(ws=None)):
        assert call(**kw) == EARG, kw
        assert b"lcr_estimate_normals" in L.lcr_last_error()
    assert call(ws_bytes=16) == ESPACE
