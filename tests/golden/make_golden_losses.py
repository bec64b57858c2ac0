"""Golden vectors for the registration loss terms from the IMPORTED reference (build container only, CPU).

    python tests/golden/make_golden_losses.py

Runs, unmodified, experiments/lcrnet/loss_reg.py (gap, node_gap, VoteLoss_new, SingleSideChamferLoss_Brute, node_overlap_Loss),
model_family/LCRNet_Matching.py's OverallLoss_new and loss_ld.py's TripletLoss on the seeded inputs of tests/losses_restatement.py (the
gap cases and the one with scored masked points), and
saves the loss values and the reference's OWN autograd gradients (fp32) with respect to the scores and the shifted nodes.  The inputs
are regenerated from their seeds by the tests; a checksum of each is saved so that a drifting generator is noticed.  For the one-sided
nearest distance at the sizes of the GPU test the reference has no class of its own shape: its `pairwise_distance` is composed the way
SingleSideChamferLoss_Brute / VoteLoss_new compose it (sqrt, min over the data, mean over the valid queries).  The distance mask of
`get_node_correspondences_disance` is saved for vote_mask.  Output: tests/golden/losses_golden.npz.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
REF = "/root/reference"


def main():
    import make_golden_model as mgm
    mgm.install_stubs()
    sys.path.insert(0, REF)
    mgm.install_ref_ext()
    import losses_restatement as R
    from experiments.lcrnet.config_model import make_cfg
    from experiments.lcrnet.loss_ld import TripletLoss
    from experiments.lcrnet.loss_reg import SingleSideChamferLoss_Brute, VoteLoss_new, gap, node_gap, node_overlap_Loss
    from experiments.lcrnet.model_family.LCRNet_Matching import OverallLoss_new
    from experiments.lcrnet.modules.ops import pairwise_distance
    from experiments.lcrnet.modules.registration.matching import get_node_correspondences_disance

    cfg = make_cfg()
    out = {}
    digest = R.digest
    for ci, c in list(enumerate(R.gap_case(shape) for shape in R.GAP_SHAPES)) + [("m", R.masked_case())]:
        out["gap%s_digest" % ci] = digest(c)
        S = R.t(c["scores"]).requires_grad_()
        losses = []
        for p in range(len(c["seg"]) - 1):
            sl = slice(c["seg"][p], c["seg"][p + 1])
            od = {"pos_node_corr_knn_points": R.t(c["p_pts"][sl]), "anc_node_corr_knn_points": R.t(c["q_pts"][sl]),
                  "pos_node_corr_knn_masks": R.t(c["pmask"][sl]), "anc_node_corr_knn_masks": R.t(c["qmask"][sl]), "matching_scores": S[sl]}
            loss = gap(cfg)(od, {"transform": R.t(c["transforms"][p])})
            losses.append(loss.item())
            if not torch.isnan(loss):
                loss.backward()
        out["gap%s_loss" % ci] = np.array(losses, np.float32)
        out["gap%s_grad" % ci] = (S.grad if S.grad is not None else torch.zeros_like(S)).numpy()
    c = R.node_case()
    out["node_digest"] = digest(c)
    S = R.t(c["scores"][0]).requires_grad_()
    loss = node_gap(cfg)({"pos_node_masks": R.t(c["pmask"][0]), "anc_node_masks": R.t(c["qmask"][0]), "gt_node_corr_indices": R.t(c["corr"]),
                          "gt_node_corr_overlaps": R.t(c["overlaps"]), "node_matching_scores": S})
    loss.backward()
    out["node_loss"], out["node_grad"] = np.float32(loss.item()), S.grad.numpy()
    for nq, nd in R.MD_SIZES:
        c = R.min_dist_case(nq, nd)
        A = R.t(c["A"]).requires_grad_()
        dist = torch.sqrt(pairwise_distance(A, R.t(c["D"]), normalized=False)).min(1)[0]
        mean = dist[R.t(c["valid"])].mean()
        mean.backward()
        tag = "md_%d_%d_" % (nq, nd)
        out[tag + "digest"], out[tag + "dist"], out[tag + "mean"], out[tag + "grad"] = digest(c), dist.detach().numpy(), np.float32(mean.item()), A.grad.numpy()
    c = R.overall_case()
    out["overall_digest"] = digest(c)
    o = R.as_tensors(c)
    ones = lambda n: torch.ones(n, dtype=torch.bool)
    mask = get_node_correspondences_disance(o["ori_pos_points_c"], o["ori_anc_points_c"], o["transform"], R.CORRES_RADIUS,
                                            ref_masks=ones(len(c["ori_pos_points_c"])), src_masks=ones(len(c["ori_anc_points_c"])))
    o["mask"] = mask
    out["overall_mask_pos"], out["overall_mask_anc"] = mask.any(1).numpy(), mask.any(0).numpy()
    res = OverallLoss_new(cfg)(o, {"transform": o["transform"]})
    res["loss"].backward()
    out["overall_keys"] = np.array(list(res.keys()))
    for k, v in res.items():
        out["overall_" + k] = np.float32(v.item())
    for k in R.GRAD_KEYS:
        out["overall_grad_" + k] = o[k].grad.numpy()
    # the terms on their own classes: the same numbers as inside OverallLoss_new, before the weights
    o2 = R.as_tensors(c, grad=False)
    o2["mask"] = mask
    out["alone_vote"] = np.float32(VoteLoss_new(cfg.Vote)(o2, {"transform": o2["transform"]}).item())
    out["alone_chamfer"] = np.float32(SingleSideChamferLoss_Brute()(o2).item())
    out["alone_node_overlap"] = np.float32(node_overlap_Loss(cfg)(o2).item())
    rng = np.random.default_rng(5)
    tri = {k: rng.normal(size=(4, n, 16)).astype(np.float32) for k, n in (("anc_global", 1), ("pos_global", 2), ("neg_global", 6))}
    out["triplet_loss"] = np.float32(TripletLoss(cfg.triplet_loss.margin)({k: R.t(v) for k, v in tri.items()})["loss"].item())
    for k, v in tri.items():
        out["triplet_" + k] = v
    path = os.path.join(HERE, "losses_golden.npz")
    np.savez_compressed(path, **out)
    print({k: float(out["overall_" + k]) for k in res}, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
