"""The registration loss terms of the reference's training / validation loop — experiments/lcrnet/loss_reg.py (gap, node_gap,
VoteLoss_new, SingleSideChamferLoss_Brute, node_overlap_Loss), model_family/LCRNet_Matching.py:359-413 (OverallLoss_new) and loss_ld.py
(TripletLoss) — under the reference's names, constructor arguments and forward signatures, on the outputs `LCRNet_Matching` returns.

The two hot terms run in HIP (csrc/losses.hip, include/lcr_hip.h): the gap loss reads the scores once and the nearest-distance terms read
the points once, both with their gradient kernels behind a torch.autograd.Function (gradient to the scores / to the queries), so
`loss.backward()` fills the .grad of torch leaf tensors.  The weighted BCE, the rotary regulariser and the triplet loss are a few tiny
torch ops on the device.  There is no model backward here: the losses are the leaves of a training path, and validate a checkpoint.
The scores they receive may carry a graph: functional.log_optimal_transport is differentiable, so matching_scores and
node_matching_scores made with grad mode on lead back to the raw scores and to the two transports' alpha.

Every module also takes the LIST of output dicts `forward_pairs` returns, with data_dict['transform'] stacked (P, 4, 4): one launch set
for all P pairs, a list of P results.  Patch counts, node counts and patch sizes may differ between the pairs.

`cfg` is the plain dict of config.make_cfg() or any object with the reference's attribute layout."""
import numpy as np
import torch
import torch.nn as nn

from . import functional as F


def _cfg(cfg, *path):
    for k in path:
        cfg = cfg[k] if isinstance(cfg, dict) else getattr(cfg, k)
    return cfg


def _pairs(output_dict):
    return (list(output_dict), True) if isinstance(output_dict, (list, tuple)) else ([output_dict], False)


def _transforms(data_dict, P, device):
    T = data_dict["transform"]
    T = torch.stack(list(T)) if isinstance(T, (list, tuple)) else T
    T = T.detach().reshape(-1, 4, 4).to(device=device, dtype=torch.float32)
    if T.shape[0] != P:
        raise RuntimeError("one transform per pair: got %d for %d pairs" % (T.shape[0], P))
    return T


def apply_transform(points, transform):
    """points (N, 3) moved by the 4x4 `transform`: points @ R^T + t."""
    return points @ transform[:3, :3].t() + transform[:3, 3]


# ---- gap core ---------------------------------------------------------------------------------------------------------------------------
class GapCore(torch.autograd.Function):
    """terms f32 [P,3] (row term, column term, mean) = lcr_gap_loss(scores, ...); gradient to `scores` only."""

    @staticmethod
    def forward(ctx, scores, geom, gamma, pmask, qmask, points, overlaps):
        saved = F.gap_loss(scores.detach(), geom, gamma, pmask, qmask, points=points, overlaps=overlaps)
        ctx.geom, ctx.gamma, ctx.saved = geom, gamma, {k: v for k, v in saved.items() if k != "terms"}
        ctx.save_for_backward(scores)
        ctx.mark_non_differentiable(saved["kept"])
        return saved["terms"], saved["kept"]

    @staticmethod
    def backward(ctx, g_terms, _g_kept):
        (scores,) = ctx.saved_tensors
        up = (g_terms[:, :2] + 0.5 * g_terms[:, 2:3]).to(torch.float32).contiguous()      # the mean is (row + column) / 2
        dS = F.gap_loss_grad(scores.detach(), ctx.geom, ctx.gamma, ctx.saved, up)
        return dS.view(scores.shape), None, None, None, None, None, None


_GEOM_CACHE = {}


def _geometry(n, m, seg, device):
    key = (tuple(n), tuple(m), tuple(seg), str(device))
    g = _GEOM_CACHE.get(key)
    if g is None:
        if len(_GEOM_CACHE) >= 64:
            _GEOM_CACHE.clear()
        g = _GEOM_CACHE[key] = F.GapGeometry(n, m, seg, device)
    return g


def _flat_scores(score_list):
    return score_list[0].reshape(-1) if len(score_list) == 1 else torch.cat([s.reshape(-1) for s in score_list])


class gap(nn.Module):
    """loss_reg.py:96-159 — the gap loss of the dense matching scores, labels from the patch points under the ground-truth transform."""

    def __init__(self, cfg):
        super().__init__()
        self.triplet_loss_gamma = _cfg(cfg, "distribution_loss", "triplet_loss_gamma")
        self.positive_radius = _cfg(cfg, "fine_loss", "positive_radius")

    def forward(self, output_dict, data_dict):
        outs, many = _pairs(output_dict)
        dev = outs[0]["matching_scores"].device
        T = _transforms(data_dict, len(outs), dev)
        n, m, seg = [], [], [0]
        for o in outs:
            b, n1, m1 = o["matching_scores"].shape
            if b < 1:
                raise RuntimeError("gap: a pair without a patch pair")
            n += [n1 - 1] * b
            m += [m1 - 1] * b
            seg.append(seg[-1] + b)
        geom = _geometry(n, m, seg, dev)
        cat = lambda k, w: (outs[0][k].reshape(-1, w) if len(outs) == 1 else torch.cat([o[k].reshape(-1, w) for o in outs])).detach()
        terms, _ = GapCore.apply(_flat_scores([o["matching_scores"] for o in outs]), geom, float(self.triplet_loss_gamma),
                                 cat("pos_node_corr_knn_masks", 1), cat("anc_node_corr_knn_masks", 1),
                                 (cat("pos_node_corr_knn_points", 3).float(), cat("anc_node_corr_knn_points", 3).float(), T,
                                  float(self.positive_radius)), None)
        return list(terms[:, 2].unbind(0)) if many else terms[0, 2]


class node_gap(nn.Module):
    """loss_reg.py:163-231 — the gap loss of the node matching scores, labels from the ground-truth node overlaps."""

    def __init__(self, cfg):
        super().__init__()
        self.triplet_loss_gamma = _cfg(cfg, "distribution_loss", "triplet_loss_gamma")
        self.positive_radius = _cfg(cfg, "coarse_loss", "positive_overlap")

    def forward(self, output_dict):
        outs, many = _pairs(output_dict)
        n = [o["node_matching_scores"].shape[0] - 1 for o in outs]
        m = [o["node_matching_scores"].shape[1] - 1 for o in outs]
        dev = outs[0]["node_matching_scores"].device
        geom = _geometry(n, m, list(range(len(outs) + 1)), dev)
        cat = lambda k: (outs[0][k] if len(outs) == 1 else torch.cat([o[k] for o in outs])).detach()
        corr = cat("gt_node_corr_indices").reshape(-1, 2).long()
        terms, _ = GapCore.apply(_flat_scores([o["node_matching_scores"] for o in outs]), geom, float(self.triplet_loss_gamma),
                                 cat("pos_node_masks"), cat("anc_node_masks"), None,
                                 (corr, cat("gt_node_corr_overlaps").float(), [o["gt_node_corr_indices"].shape[0] for o in outs],
                                  float(self.positive_radius)))
        return list(terms[:, 2].unbind(0)) if many else terms[0, 2]


# ---- nearest distance ---------------------------------------------------------------------------------------------------------------------
class MinDist(torch.autograd.Function):
    """mean f32 [P] = lcr_min_dist(A, D, ...): per segment, the mean over the valid queries of the distance to the nearest data point.
    The kernel's gradient goes to the queries A.  Where the data D are parameters too (the vote loss, whose data are the other
    cloud's shifted nodes) every query's gradient is also handed, negated, to its nearest data point: one index_add of [na, 3]."""

    @staticmethod
    def forward(ctx, A, D, a_counts, d_counts, valid):
        saved = F.min_dist(A.detach(), D.detach(), a_counts, d_counts, valid)
        ctx.saved, ctx.a_counts, ctx.d_counts = {k: v for k, v in saved.items() if k != "mean"}, a_counts, d_counts
        ctx.save_for_backward(A, D)
        return saved["mean"]

    @staticmethod
    def backward(ctx, g):
        A, D = ctx.saved_tensors
        s = ctx.saved
        dA = F.min_dist_grad(A.detach(), D.detach(), ctx.a_counts, ctx.d_counts, s, g.to(torch.float32).contiguous())
        dD = None
        if ctx.needs_input_grad[1]:
            seg = F.host_values(np.repeat(np.arange(len(ctx.a_counts)), ctx.a_counts), torch.int64, A.device)
            row = (s["d_start"].long()[seg] + s["arg"].long()).clamp(min=0)       # arg = -1 (an empty segment) carries a zero gradient
            dD = torch.zeros_like(D).index_add_(0, row, -dA)
        return (dA if ctx.needs_input_grad[0] else None), dD, None, None, None


class SingleSideChamferLoss_Brute(nn.Module):
    """loss_reg.py:21-45 — the shifted nodes of each cloud against that cloud's fine points."""

    def forward(self, output_dict):
        outs, many = _pairs(output_dict)
        A = torch.cat([o[k] for o in outs for k in ("shifted_pos_points_c", "shifted_anc_points_c")]).float()
        D = torch.cat([o[k] for o in outs for k in ("pos_points_f", "anc_points_f")]).detach().float()
        a_counts = [o[k].shape[0] for o in outs for k in ("shifted_pos_points_c", "shifted_anc_points_c")]
        d_counts = [o[k].shape[0] for o in outs for k in ("pos_points_f", "anc_points_f")]
        mean = MinDist.apply(A, D, a_counts, d_counts, None).view(-1, 2)
        loss = (mean[:, 0] + mean[:, 1]) / 2
        return list(loss.unbind(0)) if many else loss[0]


def vote_mask(ori_pos_points_c, ori_anc_points_c, transform, corres_radius):
    """The two validity vectors VoteLoss_new reads from the training-mode output 'mask' — mask.any(1), mask.any(0) of
    get_node_correspondences_disance (modules/registration/matching.py:443-516) — without the (M, N) matrix: a node is valid iff its
    nearest node of the other cloud, the anc nodes moved by `transform`, is closer than the threshold.  Like the reference, the SQUARED
    distance is compared with corres_radius itself.  d2 is taken by differences on the nearest row lcr_min_dist returns."""
    pos = ori_pos_points_c.detach().float().contiguous()
    anc = apply_transform(ori_anc_points_c.detach().float(), transform.detach().float().to(pos.device)).contiguous()
    if pos.shape[0] == 0 or anc.shape[0] == 0:
        z = lambda x: torch.zeros(x.shape[0], dtype=torch.bool, device=pos.device)
        return z(pos), z(anc)
    r = F.min_dist(torch.cat([pos, anc]), torch.cat([anc, pos]), [pos.shape[0], anc.shape[0]], [anc.shape[0], pos.shape[0]])
    arg = r["arg"].long()

    def near(a, d, idx):
        x = a - d[idx]
        return ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]).clamp(min=1e-12) < corres_radius
    return near(pos, anc, arg[:pos.shape[0]]), near(anc, pos, arg[pos.shape[0]:])


class VoteLoss_new(nn.Module):
    """loss_reg.py:48-92 — the two-sided chamfer distance between the shifted pos nodes and the transformed shifted anc nodes over the
    nodes that have a counterpart.  output_dict['mask'] is the reference's (M, N) matrix or the pair of vectors of `vote_mask`."""

    def __init__(self, cfg):
        super().__init__()
        self.NMS_radius = _cfg(cfg, "NMS_radius")

    def forward(self, output_dict, data_dict):
        outs, many = _pairs(output_dict)
        dev = outs[0]["shifted_pos_points_c"].device
        T = _transforms(data_dict, len(outs), dev)
        A, D, valid, counts = [], [], [], []
        for p, o in enumerate(outs):
            pos = o["shifted_pos_points_c"].float()
            anc = apply_transform(o["shifted_anc_points_c"].float(), T[p])
            mask = o["mask"]
            vp, va = (mask.sum(1) > 0, mask.sum(0) > 0) if torch.is_tensor(mask) else mask
            if vp.numel() != pos.shape[0] or va.numel() != anc.shape[0]:
                raise RuntimeError("VoteLoss_new: the mask is for %d x %d nodes, the shifted nodes are %d x %d"
                                   % (vp.numel(), va.numel(), pos.shape[0], anc.shape[0]))
            A += [pos, anc]
            D += [anc, pos]
            valid += [vp.reshape(-1), va.reshape(-1)]
            counts += [pos.shape[0], anc.shape[0]]
        d_counts = [counts[i ^ 1] for i in range(len(counts))]
        mean = MinDist.apply(torch.cat(A), torch.cat(D), counts, d_counts, torch.cat(valid).to(torch.uint8)).view(-1, 2)
        loss = mean[:, 0] + mean[:, 1]
        return list(loss.unbind(0)) if many else loss[0]


# ---- the small terms: torch ops on the device ---------------------------------------------------------------------------------------------
def _weighted_bce(prediction, gt):
    """BCE weighted against the class imbalance: a label's weight is the share of the OTHER class."""
    w_negative = gt.sum() / gt.shape[0]
    weights = torch.where(gt >= 0.5, 1 - w_negative, w_negative)
    return (weights * nn.functional.binary_cross_entropy(prediction, gt, reduction="none")).mean()


class node_overlap_Loss(nn.Module):
    """loss_reg.py:234-276 — weighted BCE of the node overlap score against "the node has a ground-truth correspondence"."""

    def __init__(self, cfg=None):
        super().__init__()

    def forward(self, output_dict):
        outs, many = _pairs(output_dict)
        res = []
        for o in outs:
            idx, score = o["gt_node_corr_indices"].long(), o["score"]
            pos_gt = torch.zeros(o["pos_points_c"].shape[0], device=score.device)
            anc_gt = torch.zeros(o["anc_points_c"].shape[0], device=score.device)
            pos_gt[idx[:, 0]] = 1.0
            anc_gt[idx[:, 1]] = 1.0
            res.append(_weighted_bce(score, torch.cat((pos_gt, anc_gt))))
        return res if many else res[0]


class TripletLoss(nn.Module):
    """loss_ld.py:29-58 — the descriptor triplet loss: the FARTHEST positive against every negative, hinge at `margin`, summed over the
    negatives and averaged over the batch.  Descriptors are (B, num, D) with one anchor per row."""

    def __init__(self, margin: float):
        super().__init__()
        self.margin = margin

    def forward(self, output_dict):
        anc, pos, neg = output_dict["anc_global"], output_dict["pos_global"], output_dict["neg_global"]
        positive = ((pos - anc) ** 2).sum(2).max(1)[0].view(-1, 1)
        negative = ((neg - anc) ** 2).sum(2)
        return {"loss": (self.margin + positive - negative).clamp(min=0.0).sum(1).mean()}


class OverallLoss_new(nn.Module):
    """model_family/LCRNet_Matching.py:359-413 — c_loss, g_loss (the literal 5 x the gap term), reg_loss (the rotary angles beyond pi),
    v_loss, d_loss, n_loss and their sum 'loss'."""

    def __init__(self, cfg):
        super().__init__()
        self.coarse_loss = node_gap(cfg)
        self.distribution = gap(cfg)
        self.vote_loss = VoteLoss_new(_cfg(cfg, "Vote"))
        self.node_on_pc_loss = SingleSideChamferLoss_Brute()
        self.node_overlap_loss = node_overlap_Loss(cfg)
        self.weight_coarse_loss = _cfg(cfg, "loss", "weight_coarse_loss")
        self.weight_vote_loss = _cfg(cfg, "loss", "weight_vote_loss")
        self.weight_gap_loss = _cfg(cfg, "loss", "weight_gap_loss")

    def forward(self, output_dict, data_dict):
        outs, many = _pairs(output_dict)
        coarse = self.coarse_loss(outs)
        gaps = self.distribution(outs, data_dict)
        votes = self.vote_loss(outs, data_dict)
        on_pc = self.node_on_pc_loss(outs)
        overlap = self.node_overlap_loss(outs)
        res = []
        for p, o in enumerate(outs):
            beyond = lambda e: torch.mean(torch.clamp(abs(e) - 3.1415926, 0))
            regular = (beyond(o["pos_emb"]) + beyond(o["anc_emb"])) / 2
            d = {"c_loss": self.weight_coarse_loss * coarse[p], "g_loss": 5 * gaps[p], "reg_loss": regular,
                 "v_loss": votes[p] * self.weight_vote_loss, "d_loss": on_pc[p] * self.weight_vote_loss, "n_loss": overlap[p]}
            d["loss"] = self.weight_coarse_loss * coarse[p] + 5 * gaps[p] + regular + (votes[p] + on_pc[p]) * self.weight_vote_loss + overlap[p]
            res.append(d)
        return res if many else res[0]
