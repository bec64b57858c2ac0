"""GPU: point-to-plane ICP (csrc/icp.hip, lcr_icp_point_to_plane) against the fp64 restatement of tests/icp_plane_restatement.py — step by
step, its correspondence step against point-to-point's, planted motion against point-to-point, batch against single calls, degenerate
normals — and registration.registration_icp / tools/registration_eval.py --refine icp_plane."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_plane_restatement as ipr
import icp_restatement as ir
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def scan(name):
    return np.load(os.path.join(GOLDEN, "scans", name + ".npy"))


def gpu_normals(cloud, radius=1.0, max_nn=30):
    from lcrnet_amd import functional as F
    out = F.estimate_normals(torch.from_numpy(np.asarray(cloud, np.float32)).cuda(), [len(cloud)], radius, max_nn)
    return out["normals"].cpu().numpy()


def run(pairs, r, inits, plane=True, **kw):
    """pairs [(src, tgt, tgt_normals)], inits [S,4,4] -> dict of numpy outputs of one native call"""
    from lcrnet_amd import functional as F
    cat = lambda j: torch.from_numpy(np.concatenate([np.asarray(p[j], np.float32).reshape(-1, 3) for p in pairs])).cuda()
    init = torch.from_numpy(np.asarray(inits, np.float64).reshape(-1, 4, 4)).cuda()
    sl, tl = [len(p[0]) for p in pairs], [len(p[1]) for p in pairs]
    if plane:
        out = F.icp_point_to_plane(cat(0), sl, cat(1), tl, cat(2), init, r, **kw)
    else:
        out = F.icp_point_to_point(cat(0), sl, cat(1), tl, init, r, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def planted(tgt, seed, angle=3.0, t=(0.5, -0.3, 0.1)):
    motion = ir.rigid([0.1 * seed, -0.2, 1.0], angle, t)
    src = ir.planted_scan_pair(tgt, motion, seed=seed)
    init = motion @ np.linalg.inv(ir.rigid([0, 0, 1], 1.0, [0.2, -0.15, 0.05]))     # the estimate ICP starts from: 1 deg / 0.25 m off
    return src, motion, init


def test_per_step_parity_with_the_restatement():
    """Per step k: fitness equal (the same count over the same n), rmse within 1e-12 relative (an fp64 sum of the same fp32 d² in another
    order), and T_{k+1} from the restatement's update at the kernel's T_k within 1e-9.  A and g are fp64 sums of ~1e4 terms no larger than
    |s|^2 ~ 1e4 taken in another order (relative error ~1e-13 of the largest entries); the solve of the well-conditioned 6x6 system and
    the rotation keep that far below 1e-9."""
    tgt = scan("000560")
    src, _, init = planted(tgt, 3)
    rng = np.random.default_rng(5)
    g2 = rng.uniform(-3, 3, (700, 2))
    small_t = np.concatenate([np.stack([g2[:, 0], g2[:, 1], np.zeros(700)], 1), np.stack([np.full(700, 3.0), g2[:, 0], g2[:, 1] + 3], 1),
                              np.stack([g2[:, 0], np.full(700, -3.0), g2[:, 1] + 3], 1)]).astype(np.float32)
    small_s = ir.planted_scan_pair(small_t, ir.rigid([1, 1, 1], 4.0, [0.1, 0.2, -0.1]), keep=0.8, noise=0.005, seed=6)
    pairs = [(src, tgt, gpu_normals(tgt)), (small_s, small_t, gpu_normals(small_t, 0.8))]
    inits, r = [init, np.eye(4)], 0.5
    g = run(pairs, r, inits, max_iteration=60, want_corr=True, want_history=True)
    off = 0
    for s, (ps, pt, pn) in enumerate(pairs):
        it = int(g["iterations"][s])
        assert 1 < it <= 60, it
        f, e = g["fitness_hist"][s], g["rmse_hist"][s]
        assert np.isnan(f[it + 1:]).all() and not np.isnan(f[:it + 1]).any()
        for k in range(it + 1):
            Tk = g["T_hist"][s, k]
            want = ir.correspondence_step(ps, pt, Tk, r)
            assert f[k] == want["fitness"], (s, k)
            assert abs(e[k] - want["rmse"]) <= 1e-12 * max(1.0, want["rmse"]), (s, k)
            if k < it:
                Tn, _ = ipr.plane_update(ps, pt, pn, want["corr"], Tk)
                assert np.abs(Tn - g["T_hist"][s, k + 1]).max() < 1e-9, (s, k, np.abs(Tn - g["T_hist"][s, k + 1]).max())
            if k == it:
                assert np.array_equal(g["corr"][off:off + len(ps)], want["corr"].astype(np.int32))
                assert np.array_equal(g["T"][s], Tk) and g["fitness"][s] == f[k] and g["inlier_rmse"][s] == e[k]
        stops = [ir.converged(dict(fitness=f[k], rmse=e[k]), dict(fitness=f[k + 1], rmse=e[k + 1]), 1e-6, 1e-6) for k in range(it)]
        assert not any(stops[:-1]) and (stops[-1] or it == 60), s
        off += len(ps)


def test_zero_iterations_equal_point_to_point():
    tgt = scan("000958")
    src, _, init = planted(tgt, 2)
    nrm = gpu_normals(tgt)
    a = run([(src, tgt, nrm)], 0.5, [init], max_iteration=0, want_corr=True)
    b = run([(src, tgt, nrm)], 0.5, [init], plane=False, max_iteration=0, want_corr=True)
    for k in ("T", "fitness", "inlier_rmse", "iterations", "corr"):
        assert np.array_equal(a[k], b[k]), k


def test_planted_motion_recovered_in_no_more_iterations_than_point_to_point():
    from lcrnet_amd import evaluation as ev
    import lcrnet_amd.synthetic as synthetic
    pairs, motions, inits = [], [], []
    for i in range(3):
        tgt = synthetic.synthetic_scan(40 + i)                           # raw scans, ~120 k rays
        src, motion, init = planted(tgt, i + 1)
        pairs.append((src, tgt, gpu_normals(tgt, 0.5)))
        motions.append(motion)
        inits.append(init)
    pl = run(pairs, 0.5, inits, max_iteration=100)
    pp = run(pairs, 0.5, inits, plane=False, max_iteration=100)
    msg = []
    for s, motion in enumerate(motions):
        rre, rte = ev.compute_registration_error(motion, pl["T"][s])[:2]
        rre2, rte2 = ev.compute_registration_error(motion, pp["T"][s])[:2]
        msg.append("pair %d: point-to-plane %d iterations (RRE %.4f deg, RTE %.4f m), point-to-point %d (RRE %.4f, RTE %.4f)" % (
            s, pl["iterations"][s], rre, rte, pp["iterations"][s], rre2, rte2))
        assert rre < 0.05 and rte < 0.005 and pl["fitness"][s] > 0.9, msg[-1]
    print("\n".join(msg))
    assert (pl["iterations"] <= pp["iterations"]).all(), msg


def test_batch_equals_single_calls_bitwise():
    names = ["000026", "000560", "003528", "003854"]
    pairs, inits = [], []
    for i, n in enumerate(names):
        tgt = scan(n)
        src, _, init = planted(tgt, i + 2)
        pairs.append((src, tgt, gpu_normals(tgt)))
        inits.append(init)
    kw = dict(max_iteration=40, want_corr=True, want_history=True)
    batch = run(pairs, 0.5, inits, **kw)
    off = 0
    for i, p in enumerate(pairs):
        one = run([p], 0.5, [inits[i]], **kw)
        for k in ("T", "fitness", "inlier_rmse", "iterations", "T_hist", "fitness_hist", "rmse_hist"):
            assert np.array_equal(one[k][0:1].view(np.uint8), batch[k][i:i + 1].view(np.uint8)), (i, k)
        assert np.array_equal(one["corr"], batch["corr"][off:off + len(p[0])])
        off += len(p[0])
    for ce in (0, 1, 7):
        other = run(pairs, 0.5, inits, check_every=ce, **kw)
        for k in batch:
            assert np.array_equal(other[k].view(np.uint8), batch[k].view(np.uint8)), (ce, k)
    assert (batch["iterations"] > 1).all()


def test_zero_normals_and_coplanar_target_keep_T():
    g2 = np.random.default_rng(8).uniform(-5, 5, (3000, 2))
    flat = np.stack([g2[:, 0], g2[:, 1], np.zeros(3000)], 1).astype(np.float32)
    src = flat[:1500] + np.float32(0.05)
    T0 = ir.rigid([0, 0, 1], 1.0, [0.1, 0, 0])
    tgt = scan("000026")
    src2, _, init2 = planted(tgt, 5)
    pairs = [(src, flat, gpu_normals(flat)), (src2, tgt, np.zeros_like(tgt)), (src2, tgt, gpu_normals(tgt))]
    g = run(pairs, 0.5, [T0, init2, init2], max_iteration=20)
    for s in (0, 1):                                                     # one plane (A of rank 3) / no normal at all: T is kept
        assert np.array_equal(g["T"][s], [T0, init2][s]) and g["iterations"][s] == 1, s
        assert g["fitness"][s] > 0.5
    assert not np.array_equal(g["T"][2], init2)


def test_registration_icp_point_to_plane_api():
    from lcrnet_amd import evaluation as ev
    from lcrnet_amd.registration import ICPResult, estimate_normals, icp_batched, registration_icp
    tgt = scan("003854")
    src, motion, init = planted(tgt, 9)
    nrm = estimate_normals(tgt, 1.0, 30)
    res = registration_icp(src, torch.from_numpy(tgt).cuda(), 0.5, init, max_iteration=100, estimation_method="point_to_plane",
                           target_normals=nrm)
    assert isinstance(res, ICPResult) and res.transformation.dtype == np.float64 and res.transformation.shape == (4, 4)
    assert ev.compute_registration_error(motion, res.transformation)[0] < 0.05
    c = res.correspondence_set
    assert np.array_equal(c[:, 1], ir.correspondence_step(src, tgt, res.transformation, 0.5)["corr"][c[:, 0]])
    with pytest.raises(ValueError):
        registration_icp(src, tgt, 0.5, init, estimation_method="point_to_plane")
    with pytest.raises(ValueError):
        registration_icp(src, tgt, 0.5, init, estimation_method="generalized")
    d = torch.device("cuda")
    with pytest.raises(ValueError):
        icp_batched(torch.from_numpy(src).to(d), [len(src)], torch.from_numpy(tgt).to(d), [len(tgt)], init[None], 0.5,
                    estimation_method="point_to_plane")
    default = registration_icp(src, tgt, 0.5, init, max_iteration=100)               # the default stays point-to-point
    pp = run([(src, tgt, nrm)], 0.5, [init], plane=False, max_iteration=100)
    assert np.array_equal(default.transformation, pp["T"][0])


def test_registration_eval_refine_icp_plane_end_to_end(tmp_path):
    """As test_icp_gpu's --refine icp test: stored estimates 2 deg / 0.9 m off the planted motion; --refine icp_plane (normals of
    pos_points_f on the GPU) must accept every pair and bring RRE / RTE down."""
    from lcrnet_amd import io_formats as io
    for i, n in enumerate(("000026", "000560", "003528")):
        pos = scan(n)
        anc, motion, _ = planted(pos, i + 1)
        est = motion @ np.linalg.inv(ir.rigid([0, 0, 1], 2.0, [0.6, -0.5, 0.4]))
        k = min(len(anc), 2000)
        corr_a = anc[:k]
        corr_p = ir.transform_f32(corr_a, motion)
        out = {"pos_points_f": pos, "anc_points_f": anc, "pos_points_c": pos[:64], "anc_points_c": anc[:64], "pos_corr_points": corr_p,
               "anc_corr_points": corr_a, "pos_node_corr_indices": np.zeros(0, np.int64), "anc_node_corr_indices": np.zeros(0, np.int64),
               "corr_scores": np.ones(k, np.float32), "estimated_transform": est.astype(np.float32),
               "pos_feature_global": np.zeros((1, 256), np.float32), "anc_feature_global": np.zeros((1, 256), np.float32)}
        io.save_registration(str(tmp_path), 0, 10 + i, 20 + i, out, motion)

    def ev_tool(*extra):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_eval.py"), str(tmp_path)] + list(extra),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return r.stdout, json.loads(r.stdout.strip().splitlines()[-1])

    plain_txt, plain = ev_tool("--method", "lgr")
    ref_txt, ref = ev_tool("--method", "lgr", "--refine", "icp_plane", "--pairs-per-call", "2", "--icp-iterations", "60")
    assert ref["refine"]["method"] == "icp_plane" and ref["refine"]["normal_radius"] == 1.0 and ref["refine"]["normal_max_nn"] == 30
    assert plain_txt.splitlines()[:2] == ref_txt.splitlines()[:2]
    assert plain["pairs"] == ref["pairs"] == 3
    assert ref["registration"]["RR"] == 1.0
    assert ref["registration"]["RRE"] < 0.05 and ref["registration"]["RTE"] < 0.005
    assert plain["registration"]["RRE"] > 1.0
