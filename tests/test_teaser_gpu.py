"""GPU: the TEASER-style registration (csrc/teaser.hip, lcr_teaser_registration) against the fp64 restatement of
tests/teaser_restatement.py on the planted inputs whose decision margins tests/test_teaser_cpu.py asserts: N = 0, 1, 2 (invalid), 3, 7,
65, 130, 300 in kcore mode, 65 and 130 in none mode (the cases that run the GNC loop for tens of iterations), two motions at N = 65, a
pendant row (core k_max - 1), rows with graded noise, N = 1100 with K = 600 (more rows than a selection or voting workgroup has threads,
more partials than a step has threads), K = 270 in none mode (more rows than a sweep workgroup has threads), and a ragged batch.

Equal: core numbers (they pin the edges), selected_mask, n_selected, iterations, rot_inliers, t_count, valid.  cost: 1e-9 relative.  T:
4 * 2^-24 per rotation entry and 4 * 2^-24 * max(1, |t|_inf) per translation entry of the restatement's transform rounded to fp32 — both
sides compute in fp64 and differ by summation order, far below the fp32 rounding of the output.  There is one kernel form for every
size, so no hook forces one."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import teaser_restatement as tr
from conftest import ROOT

pytestmark = pytest.mark.gpu


def run(problems, mode="kcore", max_rows=None, **kw):
    """-> dict of numpy outputs for a list of (src, ref)"""
    from lcrnet_amd import functional as F
    lens = [len(s) for s, _ in problems]
    start = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
    cat = lambda j: torch.from_numpy(np.concatenate([np.asarray(p[j], np.float32).reshape(-1, 3) for p in problems])).cuda()
    out = F.teaser_registration(cat(0), cat(1), start, inlier_selection=mode, max_rows=max_rows, want_details=True, **kw)
    torch.cuda.synchronize()
    names = ("T", "valid", "n_selected", "rot_inliers", "t_count", "iterations", "cost", "selected_mask", "core")
    return dict(zip(names, (o.cpu().numpy() for o in out)), start=np.concatenate([[0], np.cumsum(lens)]))


def problem(out, s):
    """problem s of a batch's outputs, in the restatement's keys"""
    a, b = out["start"][s], out["start"][s + 1]
    return dict(T=out["T"][s], valid=out["valid"][s], n_selected=out["n_selected"][s], rot_inliers=out["rot_inliers"][s],
                t_count=out["t_count"][s], iterations=out["iterations"][s], cost=float(out["cost"][s]),
                selected_mask=out["selected_mask"][a:b], core=out["core"][a:b])


WANT = {}


def want_for(name, data, mode):
    """the restatement's result, computed once per input"""
    if name not in WANT:
        WANT[name] = tr.teaser(data[0], data[1], inlier_selection=mode)
    return WANT[name]


def compare(got, want, name):
    assert tr.observables(got) == tr.observables(want), name
    T32 = want["T"].astype(np.float32)
    eR = np.abs(got["T"][:3, :3].astype(np.float64) - T32[:3, :3]).max()
    et = np.abs(got["T"][:3, 3].astype(np.float64) - T32[:3, 3]).max()
    ec = abs(got["cost"] - want["cost"]) / max(abs(want["cost"]), 1e-300) if want["cost"] else abs(got["cost"])
    print(name, "K %d iterations %d: dR %.2e dt %.2e dcost %.2e" % (want["n_selected"], want["iterations"], eR, et, ec))
    assert eR <= tr.T_TOL, (name, eR)
    assert et <= tr.T_TOL * max(1.0, np.abs(want["T"][:3, 3]).max()), (name, et)
    assert ec <= tr.COST_TOL, (name, ec)
    assert np.array_equal(got["T"][3], np.array([0, 0, 0, 1], np.float32))


def test_planted_inputs_equal_the_restatement():
    for name, data, mode in tr.planted_inputs():
        got = problem(run([data[:2]], mode), 0)
        compare(got, want_for(name, data, mode), name)
        if name == ("two_motions",):
            assert np.array_equal(got["selected_mask"].astype(bool), data[3]) and got["n_selected"] == 30


def ragged():
    big = tr.planted(100, 30, 1)
    return [(np.zeros((0, 3), np.float32),) * 2, tuple(x[:2] for x in tr.planted(5, 2, 0)[:2]), tr.planted(40, 25, 1)[:2], big[:2]]


@pytest.mark.parametrize("mode", ["kcore", "none"])
def test_ragged_batch_equals_single_calls_bitwise_and_repeats(mode):
    probs = ragged()
    assert [len(p[0]) for p in probs] == [0, 2, 65, 130]
    a, b = run(probs, mode), run(probs, mode)
    keys = ("T", "valid", "n_selected", "rot_inliers", "t_count", "iterations", "cost", "selected_mask", "core")
    for k in keys:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    for s, p in enumerate(probs):
        one = run([p], mode)
        ga, go = problem(a, s), problem(one, 0)
        for k in keys:
            assert np.array_equal(np.asarray(ga[k]).tobytes(), np.asarray(go[k]).tobytes()), (s, k)
        if len(p[0]) >= 65:
            compare(ga, tr.teaser(p[0], p[1], inlier_selection=mode), ("ragged", mode, s))
    for s in (0, 1):                                       # N = 0 and N = 2: invalid
        g = problem(a, s)
        assert np.array_equal(g["T"], np.eye(4, dtype=np.float32)) and g["valid"] == 0


def test_invalid_problems_return_the_identity_and_zero_counts():
    rng = np.random.default_rng(3)
    far = (rng.uniform(-40, 40, (6, 3)).astype(np.float32), rng.uniform(-40, 40, (6, 3)).astype(np.float32))
    A, _, _ = tr.graph(far[0], far[1])
    assert not A.any()                                     # six unrelated rows: no edge, k_max = 0
    good = tr.planted(5, 2, 1)[:2]
    probs = [(good[0][:n], good[1][:n]) for n in (0, 1, 2)] + [far, good]
    for mode in ("kcore", "none"):
        out = run(probs, mode)
        for s in range(4 if mode == "kcore" else 3):
            g = problem(out, s)
            assert np.array_equal(g["T"], np.eye(4, dtype=np.float32)), (mode, s)
            assert g["valid"] == 0 and g["n_selected"] == 0 and g["rot_inliers"] == 0 and g["iterations"] == 0 and g["cost"] == 0
            assert not g["t_count"].any() and not g["selected_mask"].any()
            want_core = tr.teaser(probs[s][0], probs[s][1], inlier_selection=mode)["core"]          # still the graph's
            assert np.array_equal(g["core"], want_core), (mode, s)
        compare(problem(out, 4), tr.teaser(good[0], good[1], inlier_selection=mode), ("after invalid", mode))
    # a problem above the caller's max_rows is invalid, its neighbours are not disturbed
    out = run([good, tr.planted(40, 25, 0)[:2], good], "kcore", max_rows=30)
    assert out["valid"].tolist() == [1, 0, 1] and np.array_equal(out["T"][1], np.eye(4, dtype=np.float32))
    assert np.array_equal(out["T"][0], out["T"][2])


def test_outputs_and_workspace_may_hold_anything_and_canaries_survive():
    """The entry called directly: every output and the workspace NaN-filled (all bits set) between canaries; the results are the bytes
    of the ordinary call, and nothing is written outside the tables."""
    import lcrnet_amd._lib as L
    probs = ragged()
    for mode_name, mode in (("kcore", 0), ("none", 1)):
        ref_out = run(probs, mode_name)
        lens = [len(p[0]) for p in probs]
        S, n, max_rows = len(probs), sum(lens), max(lens)
        start = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).cuda()
        src = torch.from_numpy(np.concatenate([p[0] for p in probs])).cuda()
        ref = torch.from_numpy(np.concatenate([p[1] for p in probs])).cuda()
        need = L.ws_size("lcr_teaser_ws_bytes", S, n, max_rows, mode)
        sizes = dict(T=S * 64, valid=S * 4, n_selected=S * 4, rot_inliers=S * 8, t_count=S * 12, iterations=S * 4, cost=S * 8,
                     selected_mask=n, core=n * 4, ws=need)
        PAD = 256
        offs, off = {}, PAD
        for k, b in sizes.items():
            offs[k] = off
            off += (b + PAD - 1) // PAD * PAD + PAD
        arena = torch.full((off,), 0xFF, dtype=torch.uint8).cuda()
        canary = torch.zeros(off, dtype=torch.bool)
        canary[:] = True
        for k, b in sizes.items():
            canary[offs[k]:offs[k] + b] = False
        arena[canary.cuda()] = 0xA5
        base = arena.data_ptr()
        at = lambda k: ctypes.c_void_p(base + offs[k])
        L.call.lcr_teaser_registration(L.ptr(src), L.ptr(ref), L.ptr(start), S, n, max_rows, 0.01, 1.0, 1.4, 100, 1e-12, mode, at("T"),
                                       at("valid"), at("n_selected"), at("rot_inliers"), at("t_count"), at("iterations"), at("cost"),
                                       at("selected_mask"), at("core"), at("ws"), need, L.stream_ptr(src.device))
        torch.cuda.synchronize()
        host = arena.cpu()
        assert bool((host[canary] == 0xA5).all()), mode_name
        for k in ("T", "valid", "n_selected", "rot_inliers", "t_count", "iterations", "cost", "selected_mask", "core"):
            got = host[offs[k]:offs[k] + sizes[k]].numpy()
            assert np.array_equal(got, ref_out[k].reshape(-1).view(np.uint8)), (mode_name, k)
        # a workspace one byte short is refused
        assert L.lib().lcr_teaser_registration(L.ptr(src), L.ptr(ref), L.ptr(start), S, n, max_rows, 0.01, 1.0, 1.4, 100, 1e-12, mode, at("T"),
                                               at("valid"), at("n_selected"), at("rot_inliers"), at("t_count"), at("iterations"), at("cost"),
                                               at("selected_mask"), at("core"), at("ws"), need - 1, L.stream_ptr(src.device)) != 0


def test_the_planted_mistakes_are_seen_by_the_comparison():
    """Each mistake of the restatement (but the reversed ties, which reach no output: tests/test_teaser_cpu.py) differs from the GPU's
    result in one of the equalities or by 100 x a tolerance, on an input where the correct restatement agrees with the GPU."""
    for mistake, make in tr.MISTAKE_INPUTS.items():
        (src, ref, _, _), mode = make()
        got = problem(run([(src, ref)], mode), 0)
        compare(got, tr.teaser(src, ref, inlier_selection=mode), mistake)
        wrong = tr.teaser(src, ref, inlier_selection=mode, mistake=mistake)
        got64 = dict(got, T=got["T"].astype(np.float64))
        assert tr.seen(wrong, got64), mistake


def test_parameters_reach_the_kernels():
    """Other parameters than the defaults: a wider bound with cbar2, another factor, an iteration cap that cuts the loop short."""
    src, ref, _, _ = tr.graded(0)
    for kw in (dict(noise_bound=0.02, cbar2=1.5), dict(gnc_factor=1.9), dict(max_iterations=7), dict(cost_threshold=0.0)):
        for mode in ("kcore", "none"):
            got = problem(run([(src, ref)], mode, **kw), 0)
            want = tr.teaser(src, ref, inlier_selection=mode, **kw)
            if mode == "kcore":
                assert tr.graph(src, ref, kw.get("noise_bound", 0.01), kw.get("cbar2", 1.0))[1].min() >= 1e-9
            if want["gnc"] is not None:                    # the same margins as the planted inputs, or the case proves nothing
                c2 = kw.get("noise_bound", 0.01) ** 2
                thr = kw.get("cost_threshold", 1e-12)
                assert np.abs(want["gnc"]["residuals"] - c2).min() >= 1e-6 * c2
                assert thr == 0 or all(not (thr / 10 <= h[3] <= thr * 10) for h in want["gnc"]["history"]), kw
                assert min(tr.vote_margin(v) for v in want["votes"]) >= 1e-6
            compare(got, want, (tuple(kw.items()), mode))
            if mode == "none":
                assert got["iterations"] == (7 if "max_iterations" in kw else 100 if "cost_threshold" in kw else want["iterations"])


def test_registration_with_teaser_from_correspondences_api():
    from lcrnet_amd.registration import registration_with_teaser_from_correspondences as reg
    src, ref, Tp, inl = tr.planted(30, 270, 0)
    want = want_for((30, 270, "kcore", 0), (src, ref), "kcore")
    T = reg(src, ref)
    assert T.dtype == np.float64 and T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1])
    # the planted pose within the restatement's own error (plus the fp32 rounding of the stored transform)
    err = lambda X: (np.abs(X[:3, :3] - Tp[:3, :3]).max(), np.abs(X[:3, 3] - Tp[:3, 3]).max())
    assert err(T)[0] <= err(want["T"])[0] + tr.T_TOL and err(T)[1] <= err(want["T"])[1] + tr.T_TOL * 10
    assert np.linalg.norm(src[inl].astype(np.float64) @ T[:3, :3].T + T[:3, 3] - ref[inl], axis=1).max() <= 0.01
    T2 = reg(torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda(), inlier_selection="kcore", rotation_max_iterations=50)
    assert np.array_equal(T, T2)


def test_registration_eval_teaser_end_to_end(tmp_path):
    from lcrnet_amd import io_formats as io
    for i, (ni, no) in enumerate(((40, 25), (30, 100), (30, 270))):
        src, ref, Tp, _ = tr.planted(ni, no, 0)
        pos, anc = torch.from_numpy(ref), torch.from_numpy(src)            # the anchor is registered onto the positive
        out = dict(pos_points_f=pos, anc_points_f=anc, pos_points_c=pos, anc_points_c=anc, pos_corr_points=pos, anc_corr_points=anc,
                   pos_node_corr_indices=torch.zeros((0, 2), dtype=torch.int64), anc_node_corr_indices=torch.zeros((0, 2), dtype=torch.int64),
                   corr_scores=torch.linspace(1, 0.5, len(src)), estimated_transform=torch.eye(4),
                   pos_feature_global=torch.zeros(1, 256), anc_feature_global=torch.zeros(1, 256))
        io.save_registration(str(tmp_path), 0, 100 + i, 200 + i, out, Tp)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "registration_eval.py"), str(tmp_path), "--method", "teaser",
                        "--pairs-per-call", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "Pairs: 3" and lines[1].startswith("  Fine Matching, FMR: ") and lines[2].startswith("  Registration, RR: 1.0000, RRE: ")
    got = json.loads(lines[-1])
    assert got["method"] == "teaser" and got["pairs"] == 3 and got["registration"]["RR"] == 1.0
    assert got["registration"]["RRE"] < 0.05 and got["registration"]["RTE"] < 0.01
    tz = got["teaser"]
    assert tz["invalid"] == 0 and tz["n_selected"] == pytest.approx((40 + 30 + 30) / 3) and tz["inlier_selection"] == "kcore"
    assert tz["noise_bound"] == 0.01 and tz["cbar2"] == 1.0 and tz["gnc_factor"] == 1.4 and tz["max_iterations"] == 100
    assert tz["cost_threshold"] == 1e-12
