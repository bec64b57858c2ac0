"""CPU: the fp64 restatement of the TEASER-style registration (tests/teaser_restatement.py) against the brute-force definitions of its
stages, the decision margins of the planted inputs that tests/test_teaser_gpu.py runs on the GPU, the planted mistakes, and the argument
refusals of lcr_teaser_ws_bytes / lcr_teaser_registration and of the Python entries (no launch happens: no GPU needed).

One planted mistake cannot reach the outputs: breaking endpoint ties the other way.  Only an enter and a leave endpoint of rows u, v with
x_u - x_v = 2 rho can tie with different values at stake.  The correct order then visits C + {u} (v still inside), the reversed one
C - {v}.  Every row of either set has its interval over the tie point, so the set's mean lies in [x_v, x_u]: in C + {u} one of u, v is at
least rho from the mean and removing it saves D^2 n / (n - 1) > rho^2; to C - {v} one of them can be added at D <= rho for
D^2 n / (n + 1) < rho^2.  Neither set is ever the minimiser, so xhat and t_count agree whichever way ties break;
test_reversed_ties_change_the_order_and_nothing_else shows both halves on an exact tie."""
import ctypes

import numpy as np
import pytest
import torch

import teaser_restatement as tr

NB = 0.01
C2 = NB * NB


def test_core_numbers_equal_the_subset_definition():
    rng = np.random.default_rng(0)
    seen_k = set()
    for trial in range(60):
        n = int(rng.integers(1, 11))
        A = rng.random((n, n)) < rng.choice([0.2, 0.5, 0.8])
        A = np.triu(A, 1)
        A = A | A.T
        got, want = tr.core_numbers(A), tr.core_numbers_brute(A)
        assert np.array_equal(got, want), (trial, A.astype(int))
        seen_k.update(want.tolist())
    assert len(seen_k) >= 6                                # empty graphs up to near-cliques


def tls(x, t, rho):
    return np.minimum((x - t) ** 2, rho * rho).sum()


def test_voting_minimises_the_tls_objective_over_all_run_means():
    rng = np.random.default_rng(1)
    rho = 0.01
    for trial in range(200):
        K = int(rng.integers(1, 9))
        x = np.where(rng.random(K) < 0.6, rng.uniform(-0.012, 0.012, K), rng.uniform(-1, 1, K)) + 3.0
        v = tr.vote_axis(x, rho)
        xs = np.sort(x)
        runs = [xs[a:b].mean() for a in range(K) for b in range(a + 1, K + 1)]
        best = min(tls(x, t, rho) for t in runs)
        assert v["costs"][v["best"]] == pytest.approx(best, rel=1e-9, abs=1e-18), trial
        assert tls(x, v["xhat"], rho) == pytest.approx(best, rel=1e-9, abs=1e-18), trial
        assert v["count"] == int((np.abs(x - v["xhat"]) <= rho).sum())
        assert np.all(np.diff(v["values"]) >= 0)


def test_reversed_ties_change_the_order_and_nothing_else():
    rho = 2.0 ** -7
    x = np.array([0.0, 2 * rho, rho, rho, 0.25 * rho, 5.0]) + 1.0          # enter of row 1 ties with leave of row 0, exactly
    a, b = tr.vote_axis(x, rho), tr.vote_axis(x, rho, "ties_reversed")
    assert np.array_equal(a["values"], b["values"]) and not np.array_equal(a["order"], b["order"])
    assert a["sets"] != b["sets"]
    assert a["xhat"] == b["xhat"] and a["count"] == b["count"]
    rng = np.random.default_rng(2)
    for trial in range(300):                               # random exact ties on a dyadic grid: never a different estimate
        K = int(rng.integers(2, 9))
        x = rng.integers(-6, 7, K) * (rho / 2) + 1.0
        a, b = tr.vote_axis(x, rho), tr.vote_axis(x, rho, "ties_reversed")
        assert a["count"] == b["count"] and a["costs"][a["best"]] == b["costs"][b["best"]], (trial, x)
        assert a["xhat"] == pytest.approx(b["xhat"], abs=1e-15)


def test_gnc_without_outliers_is_the_kabsch_fit_and_stops_at_iteration_0():
    for seed in range(3):
        src, ref, T, _ = tr.planted(12, 0, seed)
        g = tr.gnc_tls(src, ref)
        a, b = tr.measurements(src, ref)
        assert g["stopped_on_mu"] and g["iterations"] == 1 and len(g["history"]) == 1
        assert np.array_equal(g["R"], tr.rotation_from_H(a.T @ b))
        assert np.all(g["weights"] == 1.0) and g["rot_inliers"] == len(a)
        assert np.abs(g["R"] - T[:3, :3]).max() < 1e-4


def kabsch(src, ref):
    s, r = src.astype(np.float64), ref.astype(np.float64)
    cs, cr = s.mean(0), r.mean(0)
    R = tr.rotation_from_H((s - cs).T @ (r - cr))
    return R, cr - R @ cs


def test_planted_inputs_pose_and_decision_margins():
    """The margins under which the GPU comparison may ask for equality: they are far larger than any rounding difference between two fp64
    evaluations (1e-13 m on a length of 100 m, 1e-12 c2 on a residual, 1e-16 on a cost of 1e-2).  The voting margin is also held
    against the cancellation of the GPU's prefix differences, 4 K 2^-53 max (x - x_0)^2 (absolute, K terms in and out), by a factor 100."""
    for name, (src, ref, T, inl), mode in tr.planted_inputs():
        o = tr.teaser(src, ref, inlier_selection=mode)
        assert o["valid"] == 1, name
        if mode == "kcore":
            assert np.array_equal(o["selected_mask"].astype(bool), inl), name      # the planted inliers (the larger motion), nothing else
            assert o["edge_margins"].min() >= 1e-9, (name, o["edge_margins"].min())
        # pose: every planted inlier lands within noise_bound of its partner (the noise is within 0.2 noise_bound per axis), and the
        # rotation is the planted one to 1e-3 (millimetres of noise over baselines of metres)
        s, r = src[inl].astype(np.float64), ref[inl].astype(np.float64)
        assert np.linalg.norm(s @ o["T"][:3, :3].T + o["T"][:3, 3] - r, axis=1).max() <= NB, name
        assert np.abs(o["T"][:3, :3] - T[:3, :3]).max() < 1e-3, name
        g = o["gnc"]
        assert np.abs(g["residuals"] - C2).min() >= 1e-6 * C2, name
        for _, _, _, d in g["history"]:
            assert not (1e-13 <= d <= 1e-11), (name, d)
        if mode == "none" and len(name) == 4:
            assert 50 <= o["iterations"] <= 70 and not g["stopped_on_mu"], (name, o["iterations"])
            assert o["rot_inliers"] == inl.sum() * (inl.sum() - 1) // 2
        K = o["n_selected"]
        x = ref[o["selected"]].astype(np.float64) - src[o["selected"]].astype(np.float64) @ o["T"][:3, :3].T
        for k, v in enumerate(o["votes"]):
            m = tr.vote_margin(v)
            assert m >= 1e-9, (name, k, m)
            cancel = 4 * K * 2.0 ** -53 * np.abs(x[:, k] - x[0, k]).max() ** 2
            assert m * v["costs"][v["best"]] >= 100 * cancel, (name, k, m, cancel)


def test_plain_svd_fails_where_teaser_does_not():
    src, ref, T, inl = tr.planted(30, 270, 0)
    R, t = kabsch(src, ref)
    err = np.linalg.norm(src[inl].astype(np.float64) @ R.T + t - ref[inl], axis=1)
    assert err.min() > 1.0                                 # metres off on every inlier
    o = tr.teaser(src, ref)
    assert np.linalg.norm(src[inl].astype(np.float64) @ o["T"][:3, :3].T + o["T"][:3, 3] - ref[inl], axis=1).max() <= NB


def test_each_planted_mistake_moves_an_asserted_quantity():
    assert set(tr.MISTAKE_INPUTS) | {"ties_reversed"} == set(tr.MISTAKES)
    for mistake, make in tr.MISTAKE_INPUTS.items():
        (src, ref, _, _), mode = make()
        want, got = tr.teaser(src, ref, inlier_selection=mode), tr.teaser(src, ref, inlier_selection=mode, mistake=mistake)
        assert tr.seen(want, got), mistake
        assert not tr.seen(want, tr.teaser(src, ref, inlier_selection=mode))
    src, ref, _, _ = tr.pendant(0)
    o = tr.teaser(src, ref)
    assert sorted(o["core"].tolist()) == [1, 2, 2, 2] and o["n_selected"] == 3


def ws_bytes(S, n, max_rows, mode):
    import lcrnet_amd._lib as L
    out = ctypes.c_size_t(0)
    rc = L.lib().lcr_teaser_ws_bytes(S, n, max_rows, mode, ctypes.byref(out))
    return rc, out.value, (L.lib().lcr_last_error() or b"").decode()


def test_ws_bytes_answers_on_the_host_and_refuses_outside_the_domain():
    rc, small, _ = ws_bytes(1, 300, 300, 0)
    assert rc == 0 and small > 0
    rc, big, _ = ws_bytes(16, 16 * 4096, 4096, 0)
    assert rc == 0 and 16 * 4096 * 4096 // 8 <= big <= 16 * (4096 * 4096 // 8 + 256 * 4096)
    rc, none, _ = ws_bytes(16, 16 * 4096, 4096, 1)
    assert rc == 0 and none < big - 16 * 4096 * 4096 // 8 + 4096      # no adjacency without the graph
    assert ws_bytes(1, 0, 0, 0)[0] == 0
    for bad in [(0, 10, 10, 0), (65536, 10, 10, 0), (1, 10, 4097, 0), (1, 10, -1, 0), (1, -1, 10, 0), (2, 21, 10, 0), (1, 10, 10, 2),
                (1, 10, 10, -1)]:
        rc, _, text = ws_bytes(*bad)
        assert rc == -1 and text.startswith("lcr_teaser_ws_bytes:") and "domain" in text, bad
    import lcrnet_amd._lib as L
    assert L.lib().lcr_teaser_ws_bytes(1, 10, 10, 0, None) != 0


def test_the_entry_refuses_bad_parameters_before_any_launch():
    import lcrnet_amd._lib as L
    lib = L.lib()
    good = dict(noise_bound=0.01, cbar2=1.0, gnc_factor=1.4, max_iterations=100, cost_threshold=1e-12)
    nan, inf = float("nan"), float("inf")
    for key, values in [("noise_bound", (0.0, -1.0, nan, inf)), ("cbar2", (0.0, -1.0, nan)), ("gnc_factor", (1.0, 0.5, nan, inf)),
                        ("max_iterations", (0, 1001, -3)), ("cost_threshold", (-1e-12, nan, inf))]:
        for v in values:
            p = dict(good, **{key: v})
            rc = lib.lcr_teaser_registration(None, None, None, 1, 10, 10, p["noise_bound"], p["cbar2"], p["gnc_factor"], p["max_iterations"],
                                             p["cost_threshold"], 0, None, None, None, None, None, None, None, None, None, None, 0, None)
            assert rc == -1 and lib.lcr_last_error().startswith(b"lcr_teaser_registration:"), (key, v)
    # shape outside the domain, then null pointers: refused too
    assert lib.lcr_teaser_registration(None, None, None, 1, 10, 5000, 0.01, 1.0, 1.4, 100, 1e-12, 0, None, None, None, None, None, None, None,
                                       None, None, None, 0, None) != 0
    assert lib.lcr_teaser_registration(None, None, None, 1, 10, 10, 0.01, 1.0, 1.4, 100, 1e-12, 0, None, None, None, None, None, None, None,
                                       None, None, None, 0, None) != 0
    assert "null" in lib.lcr_last_error().decode()


def test_the_python_entries_refuse_cpu_tensors_and_bad_parameters():
    from lcrnet_amd import functional as F
    from lcrnet_amd import registration as reg
    src, ref = torch.zeros(8, 3), torch.zeros(8, 3)
    start = torch.tensor([0, 8], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="GPU only"):
        F.teaser_registration(src, ref, start)
    with pytest.raises(RuntimeError, match="GPU only"):
        reg.teaser_batched(src, ref, start)
    for kw in (dict(noise_bound=0.0), dict(cbar2=-1.0), dict(gnc_factor=1.0), dict(max_iterations=0), dict(max_iterations=1001),
               dict(cost_threshold=-1.0), dict(inlier_selection="clique"), dict(noise_bound=float("nan"))):
        with pytest.raises(ValueError):
            F.teaser_registration(src, ref, start, **kw)
    with pytest.raises(ValueError):
        reg.registration_with_teaser_from_correspondences(np.zeros((8, 3)), np.zeros((9, 3)))
    with pytest.raises(ValueError):
        reg.registration_with_teaser_from_correspondences(np.zeros((8, 3)), np.zeros((8, 3)), inlier_selection="clique")
    with pytest.raises(ValueError):
        reg.registration_with_teaser_from_correspondences(np.zeros((5000, 3)), np.zeros((5000, 3)))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            reg.registration_with_teaser_from_correspondences(np.zeros((8, 3)), np.zeros((8, 3)))
