"""GPU: the stacked-cloud table at its limits (csrc/common.h, Stack): B = 64 clouds, the last off[] slot in use, clouds 0, 31 and 63 empty.
Normals, FPFH, range images and both ICP forms give every cloud (or pair) the bits it gets in a call of its own, and empty clouds produce
nothing."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, EMPTY = 64, (0, 31, 63)
RADIUS, MAX_NN, H, W, ICP_ITERS = 0.5, 30, 16, 64, 3


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()      # bytes: NaN history rows compare equal


@pytest.fixture(scope="module")
def clouds():
    rng = np.random.default_rng(64)
    out = []
    for b in range(B):
        n = 0 if b in EMPTY else int(rng.integers(1, 41))
        out.append((np.array([5.0, 0.0, -1.0]) + rng.uniform(-0.75, 0.75, (n, 3))).astype(np.float32))
    assert [len(c) for c in out].count(0) == 3 and max(len(c) for c in out) <= 40 and sum(len(c) for c in out) < 2000
    return out


def run(clouds):
    """Every operation on `clouds` stacked in one call each; numpy outputs."""
    from lcrnet_amd import functional as F
    lens = [len(c) for c in clouds]
    S = len(clouds)
    pts = torch.from_numpy(np.concatenate(clouds).reshape(-1, 3)).cuda()
    out = {}
    nrm = F.estimate_normals(pts, lens, RADIUS, MAX_NN, want_curvature=True, want_count=True)
    out.update({"n_" + k: v for k, v in nrm.items()})
    out.update({"f_" + k: v for k, v in F.fpfh(pts, nrm["normals"], lens, RADIUS, MAX_NN, want_spfh=True, want_count=True).items()})
    out["images"], out["valid"] = F.range_images(pts, lens, H=H, W=W)
    init = torch.eye(4, dtype=torch.float64, device=pts.device).repeat(S, 1, 1)
    kw = dict(max_iteration=ICP_ITERS, want_corr=True, want_history=True)
    out.update({"p_" + k: v for k, v in F.icp_point_to_point(pts, lens, pts, lens, init, RADIUS, **kw).items()})
    out.update({"q_" + k: v for k, v in F.icp_point_to_plane(pts, lens, pts, lens, nrm["normals"], init, RADIUS, **kw).items()})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


PER_ROW = ("n_normals", "n_curvature", "n_count", "f_features", "f_spfh", "f_count", "p_corr", "q_corr")


def test_64_clouds_with_empty_ones_equal_their_own_calls(clouds):
    got = run(clouds)
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])])
    assert off[-1] == got["n_normals"].shape[0] == got["f_features"].shape[0] == got["p_corr"].shape[0]      # empty clouds own no row
    for b, cloud in enumerate(clouds):
        if b in EMPTY:
            assert (got["images"][b] == -1.0).all() and got["valid"][b] == 0
            for e in "pq":
                assert same(got[e + "_T"][b], np.eye(4)) and got[e + "_iterations"][b] == 0
                assert got[e + "_fitness"][b] == 0.0 and got[e + "_inlier_rmse"][b] == 0.0
            continue
        alone = run([cloud])
        for k in sorted(got):
            mine = got[k][off[b]:off[b + 1]] if k in PER_ROW else got[k][b:b + 1]
            assert same(mine, alone[k]), (b, k)
