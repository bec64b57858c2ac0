"""GPU: surface normals (csrc/normals.hip, lcr_estimate_normals) against the fp64 restatement of tests/normals_restatement.py — counts,
normals, degenerate sets, analytic planes, batch invariance and edge cases — and registration.estimate_normals."""
import os

import numpy as np
import pytest
import torch

import normals_restatement as nr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def scan(name):
    return np.load(os.path.join(GOLDEN, "scans", name + ".npy"))


def run(clouds, radius, max_nn, viewpoint=None):
    from lcrnet_amd import functional as F
    pts = torch.from_numpy(np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds])).cuda()
    vp = None if viewpoint is None else torch.from_numpy(np.asarray(viewpoint, np.float32).reshape(-1, 3)).cuda()
    out = F.estimate_normals(pts, [len(c) for c in clouds], radius, max_nn, vp, want_curvature=True, want_count=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(cloud, g, radius, max_nn, viewpoint=(0.0, 0.0, 0.0)):
    """g (one cloud's rows of a native call) against the restatement: counts and degenerate sets exactly, normals within 1e-6 rad where
    the eigen-gap (lam1 - lam0) > 1e-6 lam2 (up to sign where n . (v - p) is within rounding of 0), curvature within 1e-6."""
    want = nr.estimate_normals(cloud, radius, max_nn, viewpoint)
    assert np.array_equal(g["count"], want["count"])
    deg = ~g["normals"].any(axis=1)
    assert np.array_equal(deg, want["degenerate"])
    lam = want["lam"]
    ok = ~deg & (lam[:, 1] - lam[:, 0] > 1e-6 * lam[:, 2])
    n = g["normals"].astype(np.float64)
    dot = (n * want["normals"]).sum(axis=1)
    scale = np.linalg.norm(np.asarray(cloud, np.float64).reshape(-1, 3) - np.asarray(viewpoint, np.float64)[None], axis=1) + 1.0
    safe = want["dot"] > 1e-9 * scale
    # the angle from the cross product: the kernel's normal is rounded to fp32, so its length is 1 only to ~6e-8, and an arccos of the
    # dot product would read that as ~3e-4 rad; the rounding turns it by ~6e-8 rad at most
    ang = np.arctan2(np.linalg.norm(np.cross(n, want["normals"]), axis=1), np.where(safe, dot, np.abs(dot)))
    if ok.any():
        assert ang[ok].max() < 1e-6, (ang[ok].max(), int(np.argmax(np.where(ok, ang, 0))))
    assert np.abs(np.linalg.norm(n[~deg], axis=1) - 1).max(initial=0) < 1e-6
    assert np.abs(g["curvature"] - want["curvature"]).max(initial=0) < 1e-6
    return want


@pytest.mark.parametrize("name", ["000026", "003528"])
def test_demo_scans_match_the_restatement(name):
    cloud = scan(name)
    for radius, max_nn in ((0.9, 30), (1.5, 64)):
        g = run([cloud], radius, max_nn)
        compare(cloud, g, radius, max_nn)


def test_raw_scan_with_dense_near_field_balls():
    import lcrnet_amd.synthetic as synthetic
    raw = synthetic.synthetic_scan(21)
    g = run([raw], 0.5, 30)
    _, full = nr.neighbourhoods(raw, 0.5, 0)
    assert full.max() > 512, full.max()                                 # balls past the radius search's 512-row path
    want = compare(raw, g, 0.5, 30)
    assert (want["count"] == 30).mean() > 0.5
    part = raw[:40000]
    compare(part, run([part], 0.5, 128), 0.5, 128)


def test_analytic_planes_oriented_toward_the_viewpoint():
    pts, normal, _ = nr.planes_cloud(4000, seed=3)
    g = run([pts], 0.9, 30)
    assert g["normals"].any(axis=1).all()
    cosang = (g["normals"].astype(np.float64) * normal).sum(axis=1)
    assert cosang.min() > 1 - 1e-6, cosang.min()
    below = run([pts], 0.9, 30, viewpoint=[[0.0, 0.0, -50.0]])         # below the ground: its normals flip, the facade's do not
    ground = normal[:, 2] == 1.0
    facade = normal[:, 0] == -1.0
    assert (below["normals"][ground, 2] < -0.999).all()
    assert np.array_equal(below["normals"][facade], g["normals"][facade])


def test_cloud_alone_equals_any_batch_position_bitwise():
    import lcrnet_amd.synthetic as synthetic
    names = ["000026", "000560", "000958", "003528", "003854", "004481"]
    others = [scan(n) for n in names] + [synthetic.synthetic_scan(31, n_azimuth=600), scan("000026")[::3]]
    probe = synthetic.synthetic_scan(7, n_azimuth=800)
    one = run([probe], 0.5, 30)
    for pos in (0, 3, 7):
        batch = others[:pos] + [probe] + others[pos:7]
        assert len(batch) == 8
        g = run(batch, 0.5, 30)
        off = sum(len(c) for c in batch[:pos])
        for k in ("normals", "curvature", "count"):
            assert np.array_equal(g[k][off:off + len(probe)].view(np.uint8), one[k].view(np.uint8)), (pos, k)
    again = run([probe], 0.5, 30)
    for k in one:
        assert np.array_equal(again[k].view(np.uint8), one[k].view(np.uint8)), k


def test_edge_cases():
    rng = np.random.default_rng(4)
    empty = np.zeros((0, 3), np.float32)
    one_row = np.array([[1.0, 2.0, 3.0]], np.float32)
    two_rows = np.array([[1.0, 2.0, 3.0], [1.1, 2.0, 3.0]], np.float32)
    line = np.stack([np.linspace(0, 2, 50), np.linspace(0, 1, 50), np.zeros(50)], 1).astype(np.float32)
    dup = np.tile(np.array([[4.0, -1.0, 0.5]], np.float32), (40, 1))
    plane = np.concatenate([rng.uniform(-1, 1, (300, 2)), np.full((300, 1), -1.0)], 1).astype(np.float32)
    plane_dup = np.concatenate([plane, plane[:50]])                      # duplicate rows: ties on d2 are decided by the row
    clouds = [empty, one_row, two_rows, empty, line, dup, plane_dup]
    g = run(clouds, 0.5, 30)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    for i, c in enumerate(clouds):
        part = {k: v[off[i]:off[i + 1]] for k, v in g.items()}
        compare(c, part, 0.5, 30)
        if i in (1, 2, 4, 5):                                            # too few, collinear or coincident rows: degenerate
            assert not part["normals"].any() and not part["curvature"].any(), i
    for max_nn in (1, 3, 128):                                           # max_nn = 1: every row alone; 128: more than any ball holds
        compare(plane_dup, run([plane_dup], 0.5, max_nn), 0.5, max_nn)
    assert (run([plane_dup], 0.5, 1)["count"] == 1).all()


def test_registration_estimate_normals_api():
    from lcrnet_amd.registration import estimate_normals, estimate_normals_batched
    pts, normal, _ = nr.planes_cloud(1000, seed=5)
    n_np = estimate_normals(pts, 0.9)
    assert isinstance(n_np, np.ndarray) and n_np.dtype == np.float32 and n_np.shape == pts.shape
    assert ((n_np.astype(np.float64) * normal).sum(axis=1) > 1 - 1e-6).all()
    n_t = estimate_normals(torch.from_numpy(pts).cuda(), 0.9)
    assert torch.is_tensor(n_t) and n_t.is_cuda and np.array_equal(n_t.cpu().numpy(), n_np)
    with pytest.raises(ValueError):
        estimate_normals(pts, None)
    small = pts[:200]
    B = 70                                                              # more than 64 clouds: split into calls
    out = estimate_normals_batched(torch.from_numpy(np.tile(small, (B, 1))).cuda(), [len(small)] * B, 0.9, 30)
    ref = run([small], 0.9, 30)["normals"]
    got = out["normals"].cpu().numpy().reshape(B, len(small), 3)
    for i in (0, 63, 64, 69):
        assert np.array_equal(got[i], ref), i
