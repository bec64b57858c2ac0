"""GPU: generalized ICP (csrc/icp.hip, lcr_icp_generalized) against the fp64 restatement of tests/gicp_restatement.py — step by step, its
correspondence step against point-to-point's, the normal-free limits (epsilon = 1, zero normals), batch against single calls, planted
motion against point-to-point, degenerate pairs — and registration.registration_generalized_icp / tools/registration_eval.py --refine gicp."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gicp_restatement as gr
import icp_restatement as ir
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

OUT_KEYS = ("T", "fitness", "inlier_rmse", "iterations", "corr", "T_hist", "fitness_hist", "rmse_hist")


def scan(name):
    return np.load(os.path.join(GOLDEN, "scans", name + ".npy"))


def gpu_normals(cloud, radius=1.0, max_nn=30):
    from lcrnet_amd import functional as F
    out = F.estimate_normals(torch.from_numpy(np.asarray(cloud, np.float32)).cuda(), [len(cloud)], radius, max_nn)
    return out["normals"].cpu().numpy()


def planted(tgt, seed, angle=3.0, t=(0.5, -0.3, 0.1)):
    motion = ir.rigid([0.1 * seed, -0.2, 1.0], angle, t)
    src = ir.planted_scan_pair(tgt, motion, seed=seed)
    init = motion @ np.linalg.inv(ir.rigid([0, 0, 1], 1.0, [0.2, -0.15, 0.05]))     # the estimate ICP starts from: 1 deg / 0.25 m off
    return src, motion, init


@functools.lru_cache(maxsize=None)
def scan_pair(name, seed):
    """-> ((src, src_normals, tgt, tgt_normals), motion, init) of a golden scan with a planted motion; computed once, never modified"""
    tgt = scan(name)
    src, motion, init = planted(tgt, seed)
    return (src, gpu_normals(src), tgt, gpu_normals(tgt)), motion, init


def run(pairs, r, inits, eps=1e-3, gicp=True, **kw):
    """pairs [(src, src_normals, tgt, tgt_normals)], inits [S,4,4] -> dict of numpy outputs of one native call"""
    from lcrnet_amd import functional as F
    cat = lambda j: torch.from_numpy(np.concatenate([np.asarray(p[j], np.float32).reshape(-1, 3) for p in pairs])).cuda()
    init = torch.from_numpy(np.asarray(inits, np.float64).reshape(-1, 4, 4)).cuda()
    sl, tl = [len(p[0]) for p in pairs], [len(p[2]) for p in pairs]
    if gicp:
        out = F.icp_generalized(cat(0), sl, cat(1), cat(2), tl, cat(3), init, r, eps, **kw)
    else:
        out = F.icp_point_to_point(cat(0), sl, cat(2), tl, init, r, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bytes(a, b, keys=OUT_KEYS):
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def test_per_step_parity_with_the_restatement():
    """Per step k: fitness equal (the same count over the same n), rmse within 1e-12 relative (an fp64 sum of the same fp32 d² in another
    order), and T_{k+1} from the restatement's update at the kernel's T_k within 1e-9: point-to-plane's bound, by its argument.  A and g are
    fp64 sums of ~1e4 terms, each weighted by a W of norm <= 1 / (2 eps) = 500, taken in another order; the 6x6 system has a condition
    number near 1e3, so the solve and the rotation keep the difference far below 1e-9."""
    (src, sn, tgt, tn), _, init = scan_pair("000560", 3)
    rng = np.random.default_rng(5)
    g2 = rng.uniform(-3, 3, (700, 2))
    small_t = np.concatenate([np.stack([g2[:, 0], g2[:, 1], np.zeros(700)], 1), np.stack([np.full(700, 3.0), g2[:, 0], g2[:, 1] + 3], 1),
                              np.stack([g2[:, 0], np.full(700, -3.0), g2[:, 1] + 3], 1)]).astype(np.float32)
    small_s = ir.planted_scan_pair(small_t, ir.rigid([1, 1, 1], 4.0, [0.1, 0.2, -0.1]), keep=0.8, noise=0.005, seed=6)
    pairs = [(src, sn, tgt, tn), (small_s, gpu_normals(small_s, 0.8), small_t, gpu_normals(small_t, 0.8))]
    assert len(src) % 256 != 0 and len(small_s) % 256 != 0
    inits, r, eps = [init, np.eye(4)], 0.5, 1e-3
    g = run(pairs, r, inits, eps, max_iteration=60, want_corr=True, want_history=True)
    off, worst = 0, 0.0
    for s, (ps, pn, pt, qn) in enumerate(pairs):
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
                Tn, applied = gr.gicp_update(ps, pn, pt, qn, want["corr"], Tk, eps)
                diff = np.abs(Tn - g["T_hist"][s, k + 1]).max()
                worst = max(worst, diff)
                print("pair %d step %d: |T' - restatement| = %.3e" % (s, k, diff))
                assert applied and diff < 1e-9, (s, k, diff)
            if k == it:
                assert np.array_equal(g["corr"][off:off + len(ps)], want["corr"].astype(np.int32))
                assert np.array_equal(g["T"][s], Tk) and g["fitness"][s] == f[k] and g["inlier_rmse"][s] == e[k]
        stops = [ir.converged(dict(fitness=f[k], rmse=e[k]), dict(fitness=f[k + 1], rmse=e[k + 1]), 1e-6, 1e-6) for k in range(it)]
        assert not any(stops[:-1]) and (stops[-1] or it == 60), s
        off += len(ps)
    print("largest step difference %.3e" % worst)


def test_zero_iterations_equal_point_to_point():
    pair, _, init = scan_pair("000958", 2)
    a = run([pair], 0.5, [init], max_iteration=0, want_corr=True)
    b = run([pair], 0.5, [init], gicp=False, max_iteration=0, want_corr=True)
    same_bytes(a, b, ("T", "fitness", "inlier_rmse", "iterations", "corr"))
    assert a["iterations"][0] == 0 and a["fitness"][0] > 0.5


def test_eps_one_and_zero_normals_ignore_the_normals_bitwise():
    (src, sn, tgt, tn), _, init = scan_pair("000958", 2)
    kw = dict(max_iteration=30, want_corr=True, want_history=True)
    zs, zt = np.zeros_like(sn), np.zeros_like(tn)
    real = run([(src, sn, tgt, tn)], 0.5, [init], 1.0, **kw)
    none = run([(src, zs, tgt, zt)], 0.5, [init], 1.0, **kw)
    same_bytes(real, none)                                               # eps = 1: M = 2I whatever the normals
    iso = run([(src, zs, tgt, zt)], 0.5, [init], 1e-3, **kw)
    same_bytes(iso, real)                                                # zero normals: C = I on both sides, at any eps
    aniso = run([(src, sn, tgt, tn)], 0.5, [init], 1e-3, **kw)
    assert real["iterations"][0] > 1 and not np.array_equal(aniso["T"], real["T"])


def test_batch_equals_single_calls_bitwise():
    names = ["000026", "000560", "003528", "003854"]
    pairs, inits = [], []
    for i, n in enumerate(names):
        pair, _, init = scan_pair(n, i + 2)
        pairs.append(pair)
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


def test_planted_motion_recovered_in_no_more_iterations_than_point_to_point():
    from lcrnet_amd import evaluation as ev
    pairs, motions, inits = [], [], []
    for i, n in enumerate(("000026", "000560", "003528")):
        pair, motion, init = scan_pair(n, i + 1)
        pairs.append(pair)
        motions.append(motion)
        inits.append(init)
    gi = run(pairs, 0.5, inits, max_iteration=100)
    pp = run(pairs, 0.5, inits, gicp=False, max_iteration=100)
    msg = []
    for s, motion in enumerate(motions):
        rre, rte = ev.compute_registration_error(motion, gi["T"][s])[:2]
        rre2, rte2 = ev.compute_registration_error(motion, pp["T"][s])[:2]
        msg.append("pair %d: generalized %d iterations (RRE %.4f deg, RTE %.4f m, fitness %.3f), point-to-point %d (RRE %.4f, RTE %.4f)" % (
            s, gi["iterations"][s], rre, rte, gi["fitness"][s], pp["iterations"][s], rre2, rte2))
        assert rre < 0.05 and rte < 0.005 and gi["fitness"][s] > 0.9, msg[-1]
    print("\n".join(msg))
    assert (gi["iterations"] <= pp["iterations"]).all(), msg


def test_degenerate_pairs_in_one_batch():
    (src, sn, tgt, tn), _, init = scan_pair("000026", 1)
    far = (src + np.float32(100.0)).astype(np.float32)
    empty = np.zeros((0, 3), np.float32)
    pairs = [(far, sn, tgt, tn), (src[:2], sn[:2], tgt, tn), (empty, empty, tgt, tn), (src, sn, tgt, tn)]
    g = run(pairs, 0.5, [init] * 4, max_iteration=20, want_corr=True)
    assert g["fitness"][0] == 0.0 and g["inlier_rmse"][0] == 0.0 and g["iterations"][0] == 1 and np.array_equal(g["T"][0], init)
    assert (g["corr"][:len(far)] == -1).all()
    assert np.array_equal(g["T"][1], init) and g["iterations"][1] == 1                    # count < 3: the update is skipped
    assert np.array_equal(g["T"][2], init) and g["fitness"][2] == 0.0 and g["inlier_rmse"][2] == 0.0 and g["iterations"][2] == 0
    assert not np.array_equal(g["T"][3], init) and g["iterations"][3] > 1 and g["fitness"][3] > 0.9
    alone = run([pairs[3]], 0.5, [init], max_iteration=20)
    assert np.array_equal(alone["T"][0], g["T"][3])


def test_registration_generalized_icp_api():
    from lcrnet_amd import evaluation as ev
    from lcrnet_amd.registration import ICPResult, gicp_batched, registration_generalized_icp, registration_icp
    (src, sn, tgt, tn), motion, init = scan_pair("003854", 9)
    res = registration_generalized_icp(src, torch.from_numpy(tgt).cuda(), 0.5, init, max_iteration=100, source_normals=sn, target_normals=tn)
    assert isinstance(res, ICPResult) and res.transformation.dtype == np.float64 and res.transformation.shape == (4, 4)
    assert isinstance(res.fitness, float) and isinstance(res.inlier_rmse, float) and isinstance(res.iterations, int)
    assert res.correspondence_set.dtype == np.int64 and res.correspondence_set.shape[1] == 2
    rre, rte = ev.compute_registration_error(motion, res.transformation)[:2]
    assert rre < 0.05 and rte < 0.005 and res.fitness > 0.9
    c = res.correspondence_set
    assert np.array_equal(c[:, 1], ir.correspondence_step(src, tgt, res.transformation, 0.5)["corr"][c[:, 0]])
    assert len(c) == round(res.fitness * len(src))
    own = registration_generalized_icp(src, tgt, 0.5, init, max_iteration=100, normal_radius=1.0, normal_max_nn=30)
    assert np.array_equal(own.transformation.view(np.uint8), res.transformation.view(np.uint8))
    assert own.fitness == res.fitness and own.inlier_rmse == res.inlier_rmse and own.iterations == res.iterations
    assert np.array_equal(own.correspondence_set, c)
    half = registration_generalized_icp(src, tgt, 0.5, init, max_iteration=100, source_normals=sn, normal_radius=1.0)
    assert np.array_equal(half.transformation, res.transformation)
    with pytest.raises(ValueError):
        registration_generalized_icp(src, tgt, 0.5, init)
    with pytest.raises(ValueError):
        registration_generalized_icp(src, tgt, 0.5, init, source_normals=sn)
    d = torch.device("cuda")
    with pytest.raises(ValueError):
        gicp_batched(torch.from_numpy(src).to(d), [len(src)], None, torch.from_numpy(tgt).to(d), [len(tgt)], torch.from_numpy(tn).to(d),
                     init[None], 0.5)
    with pytest.raises(RuntimeError, match="lcr_icp_generalized"):
        registration_generalized_icp(src, tgt, 0.5, init, epsilon=0.0, source_normals=sn, target_normals=tn)
    default = registration_icp(src, tgt, 0.5, init, max_iteration=100)               # registration_icp is untouched: point-to-point
    pp = run([(src, sn, tgt, tn)], 0.5, [init], gicp=False, max_iteration=100)
    assert np.array_equal(default.transformation, pp["T"][0])


def test_registration_eval_refine_gicp_end_to_end(tmp_path):
    """As test_icp_plane_gpu's --refine icp_plane test: stored estimates 2 deg / 0.9 m off the planted motion; --refine gicp (normals of
    both dense clouds on the GPU) must accept every pair and bring RRE / RTE down."""
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
    ref_txt, ref = ev_tool("--method", "lgr", "--refine", "gicp", "--pairs-per-call", "2", "--icp-iterations", "60")
    assert ref["refine"]["method"] == "gicp" and ref["refine"]["epsilon"] == 1e-3
    assert ref["refine"]["normal_radius"] == 1.0 and ref["refine"]["normal_max_nn"] == 30
    assert plain_txt.splitlines()[:2] == ref_txt.splitlines()[:2]
    assert plain["pairs"] == ref["pairs"] == 3
    assert ref["registration"]["RR"] == 1.0
    assert ref["registration"]["RRE"] < 0.05 and ref["registration"]["RTE"] < 0.005
    assert plain["registration"]["RRE"] > 1.0
