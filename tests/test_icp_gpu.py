"""GPU: point-to-point ICP (csrc/icp.hip, lcr_icp_point_to_point) against the fp64 restatement of tests/icp_restatement.py — step by
step, on planted motion, batch against single calls, its correspondences against lcr_radius_query_ordered(limit = 1), edge cases inside
one batch, registration.registration_icp and tools/registration_eval.py --refine icp."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import icp_restatement as ir
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


def scan(name):
    return np.load(os.path.join(GOLDEN, "scans", name + ".npy"))


def run(pairs, r, inits, **kw):
    """pairs [(src, tgt)], inits [S,4,4] -> dict of numpy outputs of one native call"""
    from lcrnet_amd import functional as F
    cat = lambda j: torch.from_numpy(np.concatenate([np.asarray(p[j], np.float32).reshape(-1, 3) for p in pairs])).cuda()
    out = F.icp_point_to_point(cat(0), [len(p[0]) for p in pairs], cat(1), [len(p[1]) for p in pairs],
                               torch.from_numpy(np.asarray(inits, np.float64).reshape(-1, 4, 4)).cuda(), r, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def planted(tgt, seed, angle=3.0, t=(0.5, -0.3, 0.1)):
    motion = ir.rigid([0.1 * seed, -0.2, 1.0], angle, t)
    src = ir.planted_scan_pair(tgt, motion, seed=seed)
    init = motion @ np.linalg.inv(ir.rigid([0, 0, 1], 1.0, [0.2, -0.15, 0.05]))     # the estimate ICP starts from: 1 deg / 0.25 m off
    return src, motion, init


def test_per_step_parity_with_the_restatement():
    tgt = scan("000560")
    src, _, init = planted(tgt, 3)
    rng = np.random.default_rng(5)
    small_t = rng.uniform(-3, 3, (700, 3)).astype(np.float32)
    small_s = ir.planted_scan_pair(small_t, ir.rigid([1, 1, 1], 4.0, [0.1, 0.2, -0.1]), keep=0.8, noise=0.02, seed=6)
    pairs, inits, r = [(src, tgt), (small_s, small_t)], [init, np.eye(4)], 0.5
    g = run(pairs, r, inits, max_iteration=60, want_corr=True, want_history=True)
    off = 0
    for s, (ps, pt) in enumerate(pairs):
        it = int(g["iterations"][s])
        assert 1 < it <= 60, it
        f, e = g["fitness_hist"][s], g["rmse_hist"][s]
        assert np.isnan(f[it + 1:]).all() and not np.isnan(f[:it + 1]).any()
        for k in range(it + 1):
            Tk = g["T_hist"][s, k]
            want = ir.correspondence_step(ps, pt, Tk, r)
            assert f[k] == want["fitness"], (s, k)                      # same count (fitness = count / n, one division)
            assert abs(e[k] - want["rmse"]) <= 1e-12 * max(1.0, want["rmse"]), (s, k)
            if k < it:
                Tn, _ = ir.kabsch_update(ps, pt, want["corr"], Tk)
                assert np.abs(Tn - g["T_hist"][s, k + 1]).max() < 1e-9, (s, k)
            if k == it:
                assert np.array_equal(g["corr"][off:off + len(ps)], want["corr"].astype(np.int32))
                assert np.array_equal(g["T"][s], Tk) and g["fitness"][s] == f[k] and g["inlier_rmse"][s] == e[k]
        stops = [ir.converged(dict(fitness=f[k], rmse=e[k]), dict(fitness=f[k + 1], rmse=e[k + 1]), 1e-6, 1e-6) for k in range(it)]
        assert not any(stops[:-1]) and (stops[-1] or it == 60), s        # stops exactly where the rule says
        off += len(ps)
    # the correspondences at every intermediate pose: a run cut at max_iteration = k ends at T_k
    ps, pt = pairs[1]
    for k in range(0, int(g["iterations"][1]) + 1):
        cut = run([pairs[1]], r, [inits[1]], max_iteration=k, want_corr=True)
        assert np.array_equal(cut["T"][0], g["T_hist"][1, k])
        assert np.array_equal(cut["corr"], ir.correspondence_step(ps, pt, g["T_hist"][1, k], r)["corr"].astype(np.int32)), k


@pytest.mark.parametrize("which", ["demo", "synthetic_raw"])
def test_planted_motion_is_recovered(which):
    from lcrnet_amd import evaluation as ev
    if which == "demo":
        tgts = [scan(n) for n in ("000026", "003528")]
    else:
        import lcrnet_amd.synthetic as synthetic
        tgts = [synthetic.synthetic_scan(11)]                              # a raw scan, ~120 k rays
    pairs, motions, inits = [], [], []
    for i, tgt in enumerate(tgts):
        src, motion, init = planted(tgt, i + 1)
        pairs.append((src, tgt))
        motions.append(motion)
        inits.append(init)
    g = run(pairs, 0.5, inits, max_iteration=100)
    for s, motion in enumerate(motions):
        rre, rte = ev.compute_registration_error(motion, g["T"][s])[:2]
        print("%s pair %d: RRE %.4f deg RTE %.4f m fitness %.4f rmse %.4f, %d iterations" % (which, s, rre, rte, g["fitness"][s],
                                                                                               g["inlier_rmse"][s], g["iterations"][s]))
        assert rre < 0.05 and rte < 0.005 and g["fitness"][s] > 0.9


def test_batch_equals_single_calls_bitwise():
    names = ["000026", "000560", "000958", "003528", "003854"]
    pairs, inits = [], []
    for i, n in enumerate(names):
        tgt = scan(n)
        src, _, init = planted(tgt, i + 2)
        pairs.append((src, tgt))
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
    moved = run(pairs[1:] + pairs[:1], 0.5, inits[1:] + inits[:1], **kw)          # pair 0 at position 4
    for k in ("T", "fitness", "inlier_rmse", "iterations", "T_hist"):
        assert np.array_equal(moved[k][4:5].view(np.uint8), batch[k][0:1].view(np.uint8)), k
    for ce in (0, 1, 7):
        other = run(pairs, 0.5, inits, check_every=ce, **kw)
        for k in batch:
            assert np.array_equal(other[k].view(np.uint8), batch[k].view(np.uint8)), (ce, k)
    assert (batch["iterations"] > 1).all()


def test_corr_equals_the_radius_query_with_limit_one():
    from lcrnet_amd.modules.ops.radius_search import SupportGrid
    tgt = scan("004481")
    src, _, init = planted(tgt, 4)
    g = run([(src, tgt)], 0.5, [init], want_corr=True)
    q = torch.from_numpy(ir.transform_f32(src, g["T"][0])).cuda()
    grid = SupportGrid(torch.from_numpy(tgt).cuda(), torch.tensor([len(tgt)], dtype=torch.int64).cuda(), 0.5)
    nn = grid.query(q, torch.tensor([len(q)], dtype=torch.int64).cuda(), 1)[:, 0].cpu().numpy()
    want = np.where(nn < len(tgt), nn, -1).astype(np.int32)
    assert np.array_equal(g["corr"], want)
    assert (want >= 0).mean() == g["fitness"][0] > 0.9


def test_edge_cases_inside_one_batch():
    tgt = scan("000958")
    src, _, init = planted(tgt, 7)
    empty = np.zeros((0, 3), np.float32)
    T0 = ir.rigid([0, 1, 0], 5.0, [1, 2, 3])
    pairs = [(src, tgt), (empty, tgt), (src, empty), (src + np.float32(1000), tgt), (src, tgt)]
    inits = [init, T0, T0, np.eye(4), init]
    g = run(pairs, 0.5, inits, max_iteration=50, want_corr=True, want_history=True)
    n = len(src)
    for s in (1, 2):
        assert np.array_equal(g["T"][s], T0) and g["fitness"][s] == 0 and g["inlier_rmse"][s] == 0 and g["iterations"][s] == 0, s
        assert np.array_equal(g["T_hist"][s, 0], T0) and g["fitness_hist"][s, 0] == 0 and np.isnan(g["fitness_hist"][s, 1:]).all()
    assert (g["corr"][n:2 * n] == -1).all()                              # pair 2's source rows (pair 1 has none)
    # far offset: no partner within r -> T kept, converged after one (identity) update
    assert np.array_equal(g["T"][3], np.eye(4)) and g["fitness"][3] == 0 and g["iterations"][3] == 1 and (g["corr"][2 * n:3 * n] == -1).all()
    for s in (0, 4):
        want = ir.icp(src, tgt, 0.5, init, max_iteration=50)
        assert g["iterations"][s] == want["iterations"] and g["fitness"][s] == want["fitness"]
        assert np.abs(g["T"][s] - want["T"]).max() < 1e-9
    assert np.array_equal(g["T"][0], g["T"][4])
    z = run(pairs, 0.5, inits, max_iteration=0, want_corr=True)             # result_0 at init, nothing updated
    assert np.array_equal(z["T"], np.asarray(inits)) and (z["iterations"] == 0).all()
    want0 = ir.correspondence_step(src, tgt, init, 0.5)
    assert z["fitness"][0] == want0["fitness"] and np.array_equal(z["corr"][:n], want0["corr"].astype(np.int32))


def test_registration_icp_api_and_chunking():
    from lcrnet_amd import evaluation as ev
    from lcrnet_amd.registration import icp_batched, registration_icp
    tgt = scan("003854")
    src, motion, init = planted(tgt, 9)
    res = registration_icp(src, torch.from_numpy(tgt).cuda(), 0.5, init, max_iteration=100)
    assert res.transformation.dtype == np.float64 and res.transformation.shape == (4, 4)
    assert ev.compute_registration_error(motion, res.transformation)[0] < 0.05
    assert res.correspondence_set.dtype == np.int64 and res.correspondence_set.shape[1] == 2
    assert res.fitness == pytest.approx(len(res.correspondence_set) / len(src), abs=1e-15) and res.iterations > 0
    c = res.correspondence_set
    assert np.array_equal(c[:, 1], ir.correspondence_step(src, tgt, res.transformation, 0.5)["corr"][c[:, 0]])
    # more than 64 pairs: split into chunks, every pair as in a call of its own
    small_t = np.random.default_rng(1).uniform(-4, 4, (300, 3)).astype(np.float32)
    small_s = ir.planted_scan_pair(small_t, ir.rigid([0, 0, 1], 2.0, [0.1, 0, 0]), keep=0.9, noise=0.01, seed=2)
    S = 70
    dev = torch.device("cuda")
    out = icp_batched(torch.from_numpy(np.tile(small_s, (S, 1))).to(dev), [len(small_s)] * S, torch.from_numpy(np.tile(small_t, (S, 1))).to(dev),
                      [len(small_t)] * S, np.tile(np.eye(4), (S, 1, 1)), 0.5)
    one = run([(small_s, small_t)], 0.5, [np.eye(4)])
    assert out["T"].shape == (S, 4, 4)
    for i in (0, 63, 64, 69):
        assert np.array_equal(out["T"][i].cpu().numpy(), one["T"][0]), i


def test_registration_eval_refine_icp_end_to_end(tmp_path):
    """Pair files whose dense clouds are a demo scan (positive) and its planted, resampled, noisy copy (anchor); the stored estimate is
    the planted motion 2 deg / 0.9 m off.  --refine icp must keep every pair accepted and bring RRE / RTE down."""
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
    ref_txt, ref = ev_tool("--method", "lgr", "--refine", "icp", "--pairs-per-call", "2", "--icp-iterations", "60")
    assert "refine" not in plain and ref["refine"]["method"] == "icp"
    assert plain_txt.splitlines()[:2] == ref_txt.splitlines()[:2]            # Pairs and Fine Matching lines: not touched by the refinement
    assert plain["pairs"] == ref["pairs"] == 3
    assert ref["registration"]["RR"] >= plain["registration"]["RR"] and ref["registration"]["RR"] == 1.0
    assert ref["registration"]["RRE"] < 0.05 and ref["registration"]["RTE"] < 0.005
    assert plain["registration"]["RRE"] > 1.0
