"""CPU: generalized ICP without a GPU — the fp64 restatement (tests/gicp_restatement.py) on a planted motion, its covariance model and
its degenerate cases, and the host-side domain checks of lcr_icp_generalized_ws_bytes / lcr_icp_generalized."""
import ctypes
import os

import numpy as np

import gicp_restatement as gr
import icp_restatement as ir
import normals_restatement as nr
from conftest import GOLDEN

EARG, ESPACE = -1, -2


def small_pair(seed=0):
    """a three-plane corner and a planted source with normals of both sides (analytic target normals, rotated for the source)"""
    rng = np.random.default_rng(seed)
    g2 = rng.uniform(-3, 3, (300, 2))
    tgt = np.concatenate([np.stack([g2[:, 0], g2[:, 1], np.zeros(300)], 1), np.stack([np.full(300, 3.0), g2[:, 0], g2[:, 1] + 3], 1),
                          np.stack([g2[:, 0], np.full(300, -3.0), g2[:, 1] + 3], 1)]).astype(np.float32)
    tn = np.repeat(np.array([[0, 0, 1], [-1, 0, 0], [0, 1, 0]], np.float32), 300, axis=0)
    motion = ir.rigid([1, 1, 1], 2.0, [0.05, 0.1, -0.05])
    src = ((tgt.astype(np.float64) - motion[:3, 3]) @ motion[:3, :3]).astype(np.float32)
    sn = (tn.astype(np.float64) @ motion[:3, :3]).astype(np.float32)
    return src, sn, tgt, tn, motion


def test_restatement_recovers_planted_motion_in_no_more_iterations_than_point_to_point():
    from lcrnet_amd import evaluation as ev
    tgt = np.load(os.path.join(GOLDEN, "scans", "000026.npy"))
    motion = ir.rigid([0.1, -0.2, 1.0], 3.0, [0.5, -0.3, 0.1])
    src = ir.planted_scan_pair(tgt, motion, seed=1)
    init = motion @ np.linalg.inv(ir.rigid([0, 0, 1], 1.0, [0.2, -0.15, 0.05]))      # 1 deg / 0.25 m off the motion
    tn = nr.estimate_normals(tgt, 1.0, 30)["normals"].astype(np.float32)
    sn = nr.estimate_normals(src, 1.0, 30)["normals"].astype(np.float32)
    r = gr.icp(src, sn, tgt, tn, 0.5, init, eps=1e-3, max_iteration=100)
    pp = ir.icp(src, tgt, 0.5, init, max_iteration=100)
    rre, rte = ev.compute_registration_error(motion, r["T"])[:2]
    print("GICP %d iterations (RRE %.4f deg, RTE %.4f m, fitness %.3f), point-to-point %d" % (r["iterations"], rre, rte, r["fitness"],
                                                                                             pp["iterations"]))
    assert rre < 0.05 and rte < 0.005, (rre, rte)
    assert 0 < r["iterations"] <= pp["iterations"] < 100, (r["iterations"], pp["iterations"])
    f, e = r["fitness_hist"], r["rmse_hist"]
    stops = [abs(f[k + 1] - f[k]) < 1e-6 and abs(e[k + 1] - e[k]) < 1e-6 for k in range(len(f) - 1)]
    assert stops[-1] and not any(stops[:-1])


def test_covariance_is_the_eigenvalue_replaced_neighbourhood_covariance():
    """C(n) = V diag(eps, 1, 1) V^T for the eigenvectors V of the estimated covariance (ascending eigenvalues, n = the smallest one's):
    what Open3D's GICP initialisation builds from a covariance, to 1e-12."""
    pts, _, _ = nr.planes_cloud(400)
    idx, count = nr.neighbourhoods(pts, 1.0, 30)
    keep = count >= 3
    _, V = np.linalg.eigh(nr.covariances(pts, idx, count)[keep])
    for eps in (1e-3, 1e-6, 0.25):
        want = V @ np.diag([eps, 1.0, 1.0])[None] @ V.transpose(0, 2, 1)
        got = gr.covariance(V[:, :, 0], eps)
        assert got.shape == want.shape and keep.sum() > 1000
        assert np.abs(got - want).max() < 1e-12, np.abs(got - want).max()
    assert np.array_equal(gr.covariance(np.zeros(3), 1e-3), np.eye(3))                  # a degenerate row: isotropic
    assert np.array_equal(gr.covariance(np.zeros((4, 3), np.float32), 1e-3), np.tile(np.eye(3), (4, 1, 1)))
    assert np.allclose(gr.covariance([0, 0, 1], 1e-3), np.diag([1, 1, 1e-3]), rtol=0, atol=1e-15)


def test_update_ignores_the_normals_at_eps_one_and_moves_toward_the_motion():
    src, sn, tgt, tn, motion = small_pair()
    T0 = np.eye(4)
    corr = ir.correspondence_step(src, tgt, T0, 0.5)["corr"]
    assert (corr >= 0).sum() > 500
    a, ok_a = gr.gicp_update(src, sn, tgt, tn, corr, T0, 1.0)
    rng = np.random.default_rng(1)
    b, ok_b = gr.gicp_update(src, rng.normal(size=sn.shape).astype(np.float32), tgt, np.zeros_like(tn), corr, T0, 1.0)
    assert ok_a and ok_b and np.array_equal(a, b)                                        # M = 2I whatever the normals
    c, ok_c = gr.gicp_update(src, sn, tgt, tn, corr, T0, 1e-3)
    assert ok_c and not np.array_equal(a, c)
    z, _ = gr.gicp_update(src, np.zeros_like(sn), tgt, np.zeros_like(tn), corr, T0, 1e-3)
    assert np.array_equal(z, a)                                                          # zero normals: C = I on both sides, as at eps = 1
    err = lambda T: np.abs(T - motion).max()
    assert err(c) < 0.5 * err(T0) and err(a) < err(T0)
    # the reversed row order of the sums moves T' by rounding only
    rev, _ = gr.gicp_update(src, sn, tgt, tn, corr, T0, 1e-3, reverse=True)
    assert 0 <= np.abs(rev - c).max() < 1e-12


def test_update_keeps_T_below_three_partners_and_on_singular_systems():
    src, sn, tgt, tn, _ = small_pair()
    T0 = ir.rigid([0, 0, 1], 0.5, [0.01, 0, 0])
    corr = np.full(len(src), -1, np.int64)
    corr[[5, 400]] = [5, 400]
    T, applied = gr.gicp_update(src, sn, tgt, tn, corr, T0, 1e-3)
    assert not applied and np.array_equal(T, T0)
    T, applied = gr.gicp_update(src, sn, tgt, tn, np.full(len(src), -1, np.int64), T0, 1e-3)
    assert not applied and np.array_equal(T, T0)
    corr[[6, 401, 700]] = [6, 401, 700]
    T, applied = gr.gicp_update(src, sn, tgt, tn, corr, T0, 1e-3)
    assert applied and not np.array_equal(T, T0)
    same = np.full(3, 0, np.int64)                                                       # three copies of one row pair: A has rank 3
    T, applied = gr.gicp_update(np.tile(src[:1], (3, 1)), np.tile(sn[:1], (3, 1)), tgt, tn, same, T0, 1e-3)
    assert not applied and np.array_equal(T, T0)
    r = gr.icp(src[:0], sn[:0], tgt, tn, 0.5, T0)
    assert r["iterations"] == 0 and r["fitness"] == 0.0 and np.array_equal(r["T"], T0)


def test_ws_bytes_and_domain_checks_return_earg():
    from lcrnet_amd import _lib
    L = _lib.lib()
    nb, pl, pp = ctypes.c_size_t(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
    for shape in ((16, 16 * 84000, 16 * 120000), (1, 0, 0), (3, 257, 1000), (64, 64, 64)):
        assert L.lcr_icp_generalized_ws_bytes(*shape, ctypes.byref(nb)) == 0
        assert L.lcr_icp_plane_ws_bytes(*shape, ctypes.byref(pl)) == 0
        assert L.lcr_icp_ws_bytes(*shape, ctypes.byref(pp)) == 0
        assert nb.value >= pl.value >= pp.value, shape
    assert nb.value > 0
    for args in ((0, 10, 10), (65, 10, 10), (1, -1, 10), (1, 10, -1), (1, 2**31, 10), (1, 10, 2**31)):
        assert L.lcr_icp_generalized_ws_bytes(*args, ctypes.byref(nb)) == EARG, args
        assert b"lcr_icp_generalized_ws_bytes" in L.lcr_last_error()

    fake = ctypes.c_void_p(256)                                                         # non-null, never dereferenced: every case is refused on the host

    def call(S=1, lens=(10,), tl=(10,), r=0.5, eps=1e-3, it=30, ce=16, sn=fake, tn=fake, init=fake, ws_bytes=1 << 40):
        sl = np.asarray(list(lens) + [0] * 64, np.int64)
        tt = np.asarray(list(tl) + [0] * 64, np.int64)
        return L.lcr_icp_generalized(fake, sl.ctypes.data, sn, fake, tt.ctypes.data, tn, S, init, r, eps, it, 1e-6, 1e-6, fake, fake, fake, fake,
                                     None, None, None, None, ce, fake, ws_bytes, None)

    for kw in (dict(S=0), dict(S=65), dict(eps=0.0), dict(eps=2.0), dict(r=0.0), dict(sn=None), dict(tn=None), dict(ce=-1),
               dict(eps=float("nan")), dict(eps=9e-7), dict(eps=-1e-3), dict(it=-1), dict(it=100_001), dict(r=float("nan")), dict(r=1e20),
               dict(lens=(-1,)), dict(tl=(-5,)), dict(init=None)):
        assert call(**kw) == EARG, kw
        assert b"lcr_icp_generalized:" in L.lcr_last_error(), (kw, L.lcr_last_error())
    assert call(ws_bytes=16) == ESPACE
