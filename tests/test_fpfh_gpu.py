"""GPU: FPFH descriptors (csrc/fpfh.hip, lcr_fpfh) against the fp64 restatement of tests/fpfh_restatement.py — counts on every row, SPFH
votes on the rows whose votes are safe from rounding, FPFH within twice the fp32 output rounding — edge cases, batch invariance, guards, and
the learning-free chain normals -> FPFH -> feature-matching RANSAC -> ICP on a moved partial copy of a scene."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import fpfh_restatement as fr
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = [("000026", 1.5, 100), ("000026", 1.5, 32), ("003528", 1.5, 100), ("003528", 1.5, 32), ("scene", 0.6, 32)]


@functools.lru_cache(maxsize=None)
def cloud(name):
    """(points f32 [n,3], normals f32 [n,3] from lcr_estimate_normals) of a test input; computed once"""
    from lcrnet_amd import functional as F
    if name == "scene":
        pts, nrm_args = fr.scene_cloud(), (0.6, 30)
    else:
        pts, nrm_args = fr.nearest_rows(np.load(os.path.join(GOLDEN, "scans", name + ".npy"))), (0.9, 30)
    nrm = F.estimate_normals(torch.from_numpy(pts).cuda(), [len(pts)], *nrm_args)["normals"].cpu().numpy()
    return pts, nrm


@functools.lru_cache(maxsize=None)
def want(name, radius, max_nn):
    return fr.fpfh(*cloud(name), radius, max_nn)


def run(clouds, radius, max_nn):
    """clouds: [(points, normals), ...] -> dict of numpy arrays (features, spfh, count) of one native call"""
    from lcrnet_amd import functional as F
    pts = torch.from_numpy(np.concatenate([np.asarray(p, np.float32).reshape(-1, 3) for p, _ in clouds])).cuda()
    nrm = torch.from_numpy(np.concatenate([np.asarray(q, np.float32).reshape(-1, 3) for _, q in clouds])).cuda()
    out = F.fpfh(pts, nrm, [len(p) for p, _ in clouds], radius, max_nn, want_spfh=True, want_count=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def compare(g, w, what, max_unsafe=0.01):
    """g (one cloud's rows of a native call) against the restatement's dict w."""
    assert np.array_equal(g["count"], w["count"]), what
    m = w["count"][:, None]
    votes = np.rint(g["spfh"].astype(np.float64) * m / 100.0).astype(np.int64)
    s_safe, f_safe = w["safe_spfh"], w["safe_fpfh"]
    unsafe = 1.0 - f_safe.mean() if len(f_safe) else 0.0
    bad_votes = (votes != w["votes"]).any(axis=1)
    err = np.abs(g["features"].astype(np.float64) - w["features"])
    bound = 2.0 ** -23 * np.abs(w["features"]) + 1e-9
    print("%s: unsafe for FPFH %.4f; rows with other votes: %d safe, %d unsafe; worst err / bound on safe rows %.3f" % (
        what, unsafe, int((bad_votes & s_safe).sum()), int((bad_votes & ~s_safe).sum()), (err / bound)[f_safe].max(initial=0.0)))
    if max_unsafe is not None:
        assert unsafe <= max_unsafe, (what, unsafe)                   # the mask cannot hide a failure
    assert not (bad_votes & s_safe).any(), (what, np.nonzero(bad_votes & s_safe)[0][:5])
    assert np.array_equal(g["spfh"][s_safe], (w["spfh"][s_safe]).astype(np.float32)), what
    assert (err <= bound)[f_safe].all(), (what, (err / bound)[f_safe].max())
    assert np.isfinite(g["features"]).all()


@pytest.mark.parametrize("name,radius,max_nn", CASES)
def test_parity_with_the_restatement(name, radius, max_nn):
    w = want(name, radius, max_nn)
    if max_nn == 100:
        assert ((w["count"] > 64) & (w["count"] < max_nn - 1)).mean() > 0.05           # radius-limited rows with more than 64 neighbours
    elif name != "scene":
        assert (w["count"] == max_nn - 1).mean() > 0.5                               # the cap path
    compare(run([cloud(name)], radius, max_nn), w, "%s r=%g max_nn=%d" % (name, radius, max_nn))


def test_edge_cases_in_one_batched_call():
    rng = np.random.default_rng(11)
    z = np.array([[0.0, 0.0, 1.0]], np.float32)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    one = (np.array([[0.1, 0.2, 0.3]], np.float32), z)
    two = (np.array([[0.1, 0.2, 0.3], [0.3, 0.2, 0.3]], np.float32), np.array([[0, 0, 1], [0, 0.6, 0.8]], np.float32))
    base = rng.uniform(-1, 1, (300, 3)).astype(np.float32)                # all clouds overlap in space: a neighbour from another cloud
    nb = rng.normal(size=(300, 3))                                       # would change counts and votes
    nb = (nb / np.linalg.norm(nb, axis=1, keepdims=True)).astype(np.float32)
    dup = (np.concatenate([base, base[:60], base[:20]]), np.concatenate([nb, nb[:60], -nb[:20]]))
    part_zero = (base[::-1].copy(), np.where((np.arange(300) % 3 == 0)[:, None], np.float32(0), nb))
    all_dup = (np.tile(base[:1], (40, 1)), np.tile(z, (40, 1)))          # more coincident rows than max_nn
    clouds = [empty, one, two, dup, empty, part_zero, all_dup]
    g = run(clouds, 0.5, 32)
    off = np.concatenate([[0], np.cumsum([len(p) for p, _ in clouds])])
    for i, (p, q) in enumerate(clouds):
        part = {k: v[off[i]:off[i + 1]] for k, v in g.items()}
        w = fr.fpfh(p, q, 0.5, 32)
        compare(part, w, "edge cloud %d" % i, max_unsafe=None)
        assert len(p) < 100 or w["safe_spfh"].mean() > 0.5, i
    assert not g["features"][off[1]:off[2]].any() and g["count"][off[1]] == 0          # the single row: no neighbour
    assert g["count"][off[2]:off[3]].tolist() == [1, 1]
    mid = np.zeros(33, np.float32)
    mid[[5, 16, 27]] = 100.0
    tail = {k: v[off[6]:off[7]] for k, v in g.items()}
    assert tail["count"].tolist() == [31] * 32 + [32] * 8
    assert np.array_equal(tail["spfh"], np.tile(mid, (40, 1))) and np.array_equal(tail["features"], tail["spfh"])


def test_cloud_alone_equals_any_batch_position_bitwise():
    rng = np.random.default_rng(12)
    small = rng.uniform(-1, 1, (500, 3)).astype(np.float32)
    sn = rng.normal(size=(500, 3)).astype(np.float32)
    probes = [cloud("000026"), cloud("003528"), cloud("scene")]
    fill = [(small, sn), (small[:77] + np.float32(0.25), sn[:77])]
    alone = [run([c], 1.5, 100) for c in probes]
    for order in ([0, 3, 1, 4, 2], [2, 1, 4, 0, 3]):
        batch = [(probes + fill)[j] for j in order]
        g = run(batch, 1.5, 100)
        off = np.concatenate([[0], np.cumsum([len(p) for p, _ in batch])])
        for pos, j in enumerate(order):
            if j < 3:
                for k in ("features", "spfh", "count"):
                    assert np.array_equal(g[k][off[pos]:off[pos + 1]].view(np.uint8), alone[j][k].view(np.uint8)), (order, pos, k)


def test_nan_workspace_and_canary_rows():
    from lcrnet_amd import _lib
    L = _lib.lib()
    clouds = [cloud("scene"), (np.zeros((0, 3), np.float32),) * 2, cloud("000026")]
    radius, max_nn = 1.5, 100
    ref = run(clouds, radius, max_nn)
    pts = torch.from_numpy(np.concatenate([p for p, _ in clouds])).cuda()
    nrm = torch.from_numpy(np.concatenate([q for _, q in clouds])).cuda()
    ln = np.asarray([len(p) for p, _ in clouds], np.int64)
    n = int(ln.sum())
    nb = ctypes.c_size_t(0)
    assert L.lcr_fpfh_ws_bytes(len(ln), n, max_nn, ctypes.byref(nb)) == 0 and nb.value % 4 == 0
    ws = torch.empty(nb.value + 4096, dtype=torch.uint8, device="cuda")
    ws[:nb.value].view(torch.float32).fill_(float("nan"))
    ws[nb.value:].fill_(0xA5)
    feat = torch.full((n + 2, 33), -7.0, dtype=torch.float32, device="cuda")
    spfh = torch.full((n + 2, 33), -7.0, dtype=torch.float32, device="cuda")
    cnt = torch.full((n + 66,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = L.lcr_fpfh(_lib.ptr(pts), _lib.ptr(nrm), ln.ctypes.data, len(ln), radius, max_nn, ctypes.c_void_p(feat.data_ptr() + 33 * 4),
                    ctypes.c_void_p(spfh.data_ptr() + 33 * 4), ctypes.c_void_p(cnt.data_ptr() + 33 * 4), _lib.ptr(ws), nb.value,
                    _lib.stream_ptr(pts.device))
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((ws[nb.value:] == 0xA5).all())
    for t in (feat, spfh):
        assert bool((t[0] == -7.0).all()) and bool((t[-1] == -7.0).all())
    assert bool((cnt[:33] == -7).all()) and bool((cnt[33 + n:] == -7).all())
    assert np.array_equal(feat[1:-1].cpu().numpy().view(np.uint8), ref["features"].view(np.uint8))
    assert np.array_equal(spfh[1:-1].cpu().numpy().view(np.uint8), ref["spfh"].view(np.uint8))
    assert np.array_equal(cnt[33:33 + n].cpu().numpy(), ref["count"])
    assert np.isfinite(ref["features"]).all()
    assert L.lcr_fpfh(_lib.ptr(pts), _lib.ptr(nrm), ln.ctypes.data, len(ln), radius, max_nn, _lib.ptr(feat), None, None, _lib.ptr(ws),
                      nb.value - 1, _lib.stream_ptr(pts.device)) == -2


def test_registration_api_and_more_than_64_clouds():
    from lcrnet_amd.registration import compute_fpfh_feature, compute_fpfh_feature_batched
    pts, nrm = cloud("scene")
    ref = run([(pts, nrm)], 0.6, 32)["features"]
    f_np = compute_fpfh_feature(pts, nrm, 0.6, 32)
    assert isinstance(f_np, np.ndarray) and f_np.dtype == np.float32 and f_np.shape == (len(pts), 33) and np.array_equal(f_np, ref)
    f_t = compute_fpfh_feature(torch.from_numpy(pts).cuda(), torch.from_numpy(nrm).cuda(), 0.6, 32)
    assert torch.is_tensor(f_t) and f_t.is_cuda and np.array_equal(f_t.cpu().numpy(), ref)
    small_p, small_n = pts[:150], nrm[:150]
    one = run([(small_p, small_n)], 0.6, 32)["features"]
    B = 70
    out = compute_fpfh_feature_batched(torch.from_numpy(np.tile(small_p, (B, 1))).cuda(), torch.from_numpy(np.tile(small_n, (B, 1))).cuda(),
                                       [150] * B, 0.6, 32).cpu().numpy().reshape(B, 150, 33)
    for i in (0, 63, 64, 69):
        assert np.array_equal(out[i], one), i


def test_learning_free_chain_registers_a_moved_partial_copy():
    """normals -> FPFH -> exact feature NN -> checked RANSAC -> ICP on the scene and a 70 % subset of it moved by 35 degrees about a
    random axis and (3, -2, 0.5) m, the source's viewpoint moved with it.  Success by evaluation.registration_partial (RRE < 5 degrees,
    RTE < 2 m)."""
    from lcrnet_amd import evaluation
    from lcrnet_amd.registration import fpfh_ransac_batched, icp_batched
    scene = fr.scene_cloud()
    rng = np.random.default_rng(7)
    sub = np.sort(rng.choice(len(scene), int(0.7 * len(scene)), replace=False))
    R, t = fr.rotation(rng.normal(size=3), 35.0), np.array([3.0, -2.0, 0.5])
    src = (scene[sub].astype(np.float64) @ R.T + t).astype(np.float32)
    gt = np.eye(4)
    gt[:3, :3], gt[:3, 3] = R.T, -R.T @ t                                # src onto ref
    s, r = torch.from_numpy(src).cuda(), torch.from_numpy(scene).cuda()
    out = fpfh_ransac_batched(s, [len(src)], r, [len(scene)], 0.6, 30, 0.6, 32, src_viewpoint=t[None].astype(np.float32),
                              distance_threshold=0.1, num_iterations=50000)
    icp = icp_batched(s, [len(src)], r, [len(scene)], out["T"].double(), 0.3, max_iteration=30)
    torch.cuda.synchronize()
    T0, T1 = out["T"][0].cpu().numpy().astype(np.float64), icp["T"][0].cpu().numpy()
    e0, e1 = evaluation.compute_registration_error(gt, T0), evaluation.compute_registration_error(gt, T1)
    print("RANSAC: RRE %.3f deg RTE %.3f m, %d inliers of %d correspondences; after ICP: RRE %.4f deg RTE %.4f m, fitness %.3f" % (
        e0[0], e0[1], int(out["inliers"][0]), int(out["num_corr"][0]), e1[0], e1[1], float(icp["fitness"][0])))
    assert evaluation.registration_partial([gt], [T0])[1] == 1.0
    assert evaluation.registration_partial([gt], [T1])[1] == 1.0


def test_registration_eval_fpfh_ransac_needs_only_the_dense_points(tmp_path, capsys):
    """tools/registration_eval.py --method fpfh_ransac on pair files that hold nothing but pos_points_f / anc_points_f and the ground truth
    (run in this process: the tool's main takes its argv)."""
    import importlib.util
    import json
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("registration_eval_tool", os.path.join(root, "tools", "registration_eval.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    scene = fr.scene_cloud()
    for i, (seed, deg) in enumerate(((7, 35.0), (8, 20.0))):
        rng = np.random.default_rng(seed)
        sub = np.sort(rng.choice(len(scene), int(0.7 * len(scene)), replace=False))
        R, t = fr.rotation(rng.normal(size=3), deg), np.array([0.3, -0.2, 0.1])   # the viewpoint stays near the sensor: the tool assumes the origin
        gt = np.eye(4)
        gt[:3, :3], gt[:3, 3] = R.T, -R.T @ t
        np.savez(str(tmp_path / ("0_%d_%d.npz" % (i, i + 50))), pos_points_f=scene,
                 anc_points_f=(scene[sub].astype(np.float64) @ R.T + t).astype(np.float32), transform=gt)
    argv = [str(tmp_path), "--method", "fpfh_ransac", "--normal-radius", "0.6", "--fpfh-radius", "0.6", "--fpfh-max-nn", "32",
            "--distance-threshold", "0.1", "--refine", "icp", "--icp-distance", "0.3"]
    out = tool.main(argv)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["method"] == "fpfh_ransac" and line["fpfh_ransac"]["fpfh_radius"] == 0.6 and line["fpfh_ransac"]["fpfh_max_nn"] == 32
    assert line["fpfh_ransac"]["normal_radius"] == 0.6 and line["fpfh_ransac"]["normal_max_nn"] == 30
    print(line["registration"], line["fpfh_ransac"]["num_corr"])
    assert out["pairs"] == 2 and out["accepted"] == 2 and out["registration"]["RRE"] < 1.0
    with pytest.raises(SystemExit):
        np.savez(str(tmp_path / "0_9_99.npz"), pos_points_f=scene, transform=np.eye(4))
        tool.main(argv)
