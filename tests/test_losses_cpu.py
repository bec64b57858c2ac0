"""CPU: the restatement of the registration loss terms (tests/losses_restatement.py) against goldens of the IMPORTED reference modules
(tests/golden/make_golden_losses.py), the margins of every seeded input, the planted mistakes, and the torch-only modules of
lcrnet_amd.losses (TripletLoss, node_overlap_Loss, the module tree and config keys of OverallLoss_new).

The reference runs in fp32 and the restatement in fp64, so they differ by the reference's own rounding error e_ref, which is what the
GPU tests' tolerance rule is built on.  Here e_ref itself is bounded by reasoning: the gap terms are sums of <= 201 fp32 values of size
<= ~50 followed by a log and a mean (relative 201 * 2^-24 = 1.2e-5 at the very worst), their gradients are ratios of such sums; the
nearest distances of the reference come from |x|^2 - 2 x.y + |y|^2 at ~85 m from the origin, whose three terms of ~7e3 m^2 round to
~5e-4 m^2 each, i.e. up to ~2e-3 m^2 in d2 and sqrt(2e-3) = 0.045 m in a distance that is itself smaller than that."""
import numpy as np
import pytest
import torch

import losses_restatement as R
import lcrnet_amd.losses as L
from lcrnet_amd.config import make_cfg


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


def check_case_margins(kind, key=None):
    """The margin helper on one seeded input (also run by the GPU tests on each of theirs)."""
    c, r = R.cached(kind, key)
    if kind == "gap":
        for p, core in enumerate(r["pairs"]):
            R.assert_margins(d2=core["decision"], radius=R.RADIUS, cores=[core])
    elif kind == "node":
        R.assert_margins(overlaps=R.t(c["overlaps"]), thr=R.THR, cores=r["pairs"])
    elif kind == "md":
        _, _, part = R.nearest_rows(R.t(c["A"]), R.t(c["D"]))
        R.assert_margins(nearest=part, tie_rows=c["tie_rows"])
    return c, r


def test_seeded_inputs_are_the_ones_the_golden_was_made_from(gold):
    cases = {"gap%d" % ci: R.gap_case(s) for ci, s in enumerate(R.GAP_SHAPES)}
    cases.update({"gapm": R.masked_case(), "node": R.node_case(), "overall": R.overall_case()})
    cases.update({"md_%d_%d" % k: R.min_dist_case(*k) for k in R.MD_SIZES})
    for name, c in cases.items():
        assert R.digest(c) == gold[name + "_digest"], name


@pytest.mark.parametrize("ci", range(len(R.GAP_SHAPES)))
def test_gap_restatement_equals_the_reference(gold, ci):
    c, r = check_case_margins("gap", ci)
    want = gold["gap%d_loss" % ci]
    e = R.err(r["terms"][:, 2], want)                                # NaN where the reference is NaN: the fully padded pair
    eg = R.err(r["grad"], gold["gap%d_grad" % ci])
    print("gap %s: e_ref loss %.3g grad %.3g" % (R.GAP_SHAPES[ci], e, eg))
    assert e <= 1.2e-5 * max(1.0, np.nanmax(np.abs(want))) and eg <= 1.2e-5 * max(np.abs(r["grad"]).max(), 1e-30)
    if len(c["seg"]) > 2:
        assert np.isnan(want[-1]) and np.isnan(r["terms"][-1, 0]) and not np.isnan(r["terms"][-1, 1])


def test_masked_points_with_scores_equal_the_reference(gold):
    c, r = check_case_margins("gap", "masked")
    assert R.err(r["terms"][:, 2], gold["gapm_loss"]) <= 1.2e-5 * np.abs(gold["gapm_loss"]).max()
    assert R.err(r["grad"], gold["gapm_grad"]) <= 1.2e-5 * np.abs(r["grad"]).max()


def test_node_gap_restatement_equals_the_reference(gold):
    c, r = check_case_margins("node")
    e, eg = R.err(r["terms"][0, 2], gold["node_loss"]), R.err(r["grad"][0], gold["node_grad"])
    print("node gap: e_ref loss %.3g grad %.3g" % (e, eg))
    assert e <= 1.2e-5 * abs(gold["node_loss"]) and eg <= 1.2e-5 * np.abs(r["grad"]).max()
    assert r["pairs"][0]["row"]["posf"][0, 3, -1] and r["pairs"][0]["row"]["count"][0, 3] == 1      # node 3: only the dustbin is positive


@pytest.mark.parametrize("size", R.MD_SIZES)
def test_min_dist_restatement_equals_the_reference(gold, size):
    c, r = check_case_margins("md", size)
    tag = "md_%d_%d_" % size
    e = R.err(r["dist"], gold[tag + "dist"])
    print("min dist %s: e_ref dist %.3g mean %.3g grad %.3g" % (size, e, R.err(r["mean"], gold[tag + "mean"]), R.err(r["grad"], gold[tag + "grad"])))
    assert e <= 0.045
    if c["tie_rows"]:
        assert r["arg"][0] == 0                                      # the exact tie goes to the lower row
    none = R.min_dist(R.t(c["A"]), R.t(c["D"]), torch.zeros(len(c["A"]), dtype=torch.bool))[2]
    assert torch.isnan(none)                                         # no valid query: NaN, like the reference's mean of nothing


def test_overall_restatement_has_the_reference_keys_weights_and_values(gold):
    c, r = R.cached("overall")
    assert list(r["losses"]) == gold["overall_keys"].tolist() == ["c_loss", "g_loss", "reg_loss", "v_loss", "d_loss", "n_loss", "loss"]
    for k, v in r["losses"].items():
        tol = 0.25 * 0.045 if k in ("v_loss", "d_loss", "loss") else 1.2e-5 * max(1.0, abs(v))
        assert abs(v - float(gold["overall_" + k])) <= tol, k
    # the weights: the terms the reference's own classes return alone, times the weights, are the entries
    assert abs(float(gold["alone_vote"]) * 0.25 - float(gold["overall_v_loss"])) < 1e-6
    assert abs(float(gold["alone_chamfer"]) * 0.25 - float(gold["overall_d_loss"])) < 1e-6
    assert abs(float(gold["alone_node_overlap"]) - float(gold["overall_n_loss"])) < 1e-6
    for k in R.GRAD_KEYS:
        tol = 0.05 * np.abs(r["grads"][k]).max() if "shifted" in k else 1.2e-5 * np.abs(r["grads"][k]).max()
        assert R.err(r["grads"][k], gold["overall_grad_" + k]) <= tol, k
    assert np.array_equal(r["valid"][0], gold["overall_mask_pos"]) and np.array_equal(r["valid"][1], gold["overall_mask_anc"])


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_planted_mistakes_move_the_restatement_away_from_the_reference(gold, mistake):
    """Each planted mistake changes a restated loss by far more than the reference's own error: the goldens can see it."""
    if mistake == "ge_at_4r2":
        c = R.tie_case()
        a, b = R.gap_results(None, case=c)[1]["terms"][0, 2], R.gap_results(None, mistake=mistake, case=c)[1]["terms"][0, 2]
        assert abs(a - b) > 1e-3
        return
    seen = False
    for ci in ("masked", 1, 2):
        _, r = R.gap_results(ci, mistake=mistake) if ci != "masked" else R.gap_results(None, mistake=mistake, case=R.masked_case())
        want = gold["gap%s_loss" % ("m" if ci == "masked" else ci)].astype(np.float64)
        got = r["terms"][:, 2]
        seen |= not np.array_equal(np.isnan(got), np.isnan(want)) or bool((np.abs(np.nan_to_num(got) - np.nan_to_num(want)) > 1e-3).any())
    assert seen


def test_torch_only_modules_and_config(gold):
    cfg = make_cfg()
    assert cfg["coarse_loss"]["positive_overlap"] == 0.1 and cfg["fine_loss"]["positive_radius"] == 0.45
    assert cfg["distribution_loss"]["triplet_loss_gamma"] == 0.5 and cfg["triplet_loss"]["margin"] == 0.5
    assert cfg["loss"] == {"weight_coarse_loss": 1.0, "weight_vote_loss": 0.25, "weight_gap_loss": 5} and cfg["Vote"]["NMS_radius"] == 2.4
    assert cfg["model"]["ground_truth_corres_radius"] == 2.4
    m = L.OverallLoss_new(cfg)
    assert [n for n, _ in m.named_children()] == ["coarse_loss", "distribution", "vote_loss", "node_on_pc_loss", "node_overlap_loss"]
    assert (m.weight_coarse_loss, m.weight_vote_loss, m.weight_gap_loss) == (1.0, 0.25, 5)
    assert m.distribution.positive_radius == 0.45 and m.coarse_loss.positive_radius == 0.1 and m.vote_loss.NMS_radius == 2.4
    tri = {k: torch.from_numpy(gold["triplet_" + k]) for k in ("anc_global", "pos_global", "neg_global")}
    assert abs(float(L.TripletLoss(cfg["triplet_loss"]["margin"])(tri)["loss"]) - float(gold["triplet_loss"])) < 1e-5 * float(gold["triplet_loss"])
    o = R.as_tensors(R.overall_case(), grad=False)
    assert abs(float(L.node_overlap_Loss(cfg)(o)) - float(gold["alone_node_overlap"])) < 1e-6
    with pytest.raises(RuntimeError):                                # no CPU fallback for the native terms
        L.SingleSideChamferLoss_Brute()(o)
