"""LCRNet_Matching — experiments/lcrnet/model_family/LCRNet_Matching.py:25-355, the class the registration evaluation harness
builds (`experiments/registration/test_loop_closure.py:13`, BASELINE configs[4]).  Relative to `LCRNet` it has no NetVLAD head and,
in eval mode, additionally returns what the harness' Evaluator / loss terms read:

  pos_emb, anc_emb                     rotary angles of both clouds, (1, N, 64)         (:130-136, :331-332)
  score                                sigmoid(proj_node_overlap_score(node feats)) clamped to [0, 1], one per voted node (:146-147)
  node_matching_scores, pos/anc_node_masks, matching_scores                              (:212-214, :274)
  gt_node_corr_indices / _overlaps     ground-truth node correspondences under data_dict['transform'] (:189-204)

Same module tree -> same `state_dict` keys as the reference class (354 tensors, tests/test_checkpoint_layout.py).  Forward = the HIP path of
`LCRNet`.

Training mode runs the reference's training branch (:189-330) for P >= 1 pairs per call over the same batched launches, with a graph to every
parameter: the patches are those of ground-truth node correspondences drawn by `coarse_target` (SuperPointTargetGenerator, :222-224), there is
no patch matching and no registration (:277), and the output carries what `losses.OverallLoss_new` reads — `mask` for the vote loss
(:320-328, as the two vectors of losses.vote_mask), `score`, the two score tensors, the rotary angles, the shifted nodes."""
import torch

from .. import functional as F
from ..modules.registration import SuperPointTargetGenerator, get_node_correspondences, get_node_correspondences_batched
from .LCRNet import LCRNet


class LCRNet_Matching(LCRNet):
    global_head = False
    matching_extras = True

    def __init__(self, cfg=None):
        super().__init__(cfg)
        from ..config import make_cfg
        cfg = cfg or make_cfg()
        m = cfg["model"]
        self.matching_radius = m.get("ground_truth_matching_radius", 0.45)
        self.corres_radius = m.get("ground_truth_corres_radius", 2.4)
        cm = cfg.get("coarse_matching", {})
        self.coarse_target = SuperPointTargetGenerator(cm.get("num_targets", 128), cm.get("overlap_threshold", 0.1), seed=cfg.get("seed", 0))

    def forward(self, data_dict, pose=True):
        return self.forward_pairs(data_dict, pose)[0]

    def forward_pairs(self, data_dict, pose=True):
        """data_dict['transform']: (4, 4) for one pair, (P, 4, 4) or a list for P pairs per call."""
        if "transform" not in data_dict:
            raise KeyError("transform")                              # the reference reads it first thing (LCRNet_Matching.py:301)
        T = data_dict["transform"]
        T = torch.stack(list(T)) if isinstance(T, (list, tuple)) else T
        T = T.detach().reshape(-1, 4, 4).float()
        if self.training:
            return self._forward_pairs_train(data_dict, pose, T)
        outs = super().forward_pairs(data_dict, pose)
        if T.shape[0] != len(outs):
            raise RuntimeError("one transform per pair: got %d for %d pairs" % (T.shape[0], len(outs)))
        if not pose:
            return outs
        w, b = self.proj_node_overlap_score.weight, self.proj_node_overlap_score.bias
        for p, o in enumerate(outs):
            o["score"] = torch.sigmoid(F.linear(o["feats_c"].contiguous(), w, b).view(-1)).clamp(0, 1)
            N_pos, N_anc = o["pos_points_f"].shape[0], o["anc_points_f"].shape[0]
            pad = lambda x: torch.cat([x, torch.zeros_like(x[:1])], 0)
            pos_knn_pts = pad(o["pos_points_f"])[o["pos_node_knn_indices"].clamp(max=N_pos)]
            anc_knn_pts = pad(o["anc_points_f"])[o["anc_node_knn_indices"].clamp(max=N_anc)]
            gi, go = get_node_correspondences(o["pos_points_c"], o["anc_points_c"], pos_knn_pts, anc_knn_pts, T[p].to(pos_knn_pts.device),
                                              self.matching_radius, o["pos_node_masks"], o["anc_node_masks"], o["pos_node_knn_masks"],
                                              o["anc_node_knn_masks"])
            o["gt_node_corr_indices"], o["gt_node_corr_overlaps"] = gi, go
        return outs

    # ---- the training branch (LCRNet_Matching.py:189-330) -------------------------------------------------------------------------------
    def _forward_pairs_train(self, data_dict, pose, T):
        P = data_dict["lengths"][-1].numel() // 2
        if T.shape[0] != P:
            raise RuntimeError("one transform per pair: got %d for %d pairs" % (T.shape[0], P))
        T = T.to(data_dict["points"][0].device)
        with torch.enable_grad():
            outs = self._forward_pairs(data_dict, pose, True, T)
        if pose:
            from ..losses import vote_mask
            for p, o in enumerate(outs):
                o["mask"] = vote_mask(o["ori_pos_points_c"], o["ori_anc_points_c"], T[p], self.corres_radius)       # :320-328
        return outs

    def _dense_matching_train(self, outs, P, pts_f, feats_f, off_f, vd, off_m, T):
        """DenseMatchingHEAD in training mode for P pairs: the partition and the node-level transport of the inference group path (with a
        graph: bmm_nt and the transport carry backwards), ground-truth node correspondences per pair (no gradient), `coarse_target`'s
        selection, the patch gathers over the whole stack and the patch-level transport of all selected pairs in one call
        (_PatchTransportFn: lcr_patch_scores forward, lcr_patch_scores_grad backward).  A pair without a correspondence above the overlap
        threshold raises: the gap loss has no meaning on an empty patch batch."""
        parts, nm_all, knn_all, km_all, m, Mx, Nx, tab, ns = self._node_transport_group(P, pts_f, off_f, vd, off_m)
        fc, nodes = vd["feats_c"], vd["points_c"]
        labels = [{"pos_points_f": pts_f[off_f[2 * p]:off_f[2 * p + 1]], "anc_points_f": pts_f[off_f[2 * p + 1]:off_f[2 * p + 2]],
                   "pos_points_c": nodes[off_m[2 * p]:off_m[2 * p + 1]].detach(), "anc_points_c": nodes[off_m[2 * p + 1]:off_m[2 * p + 2]].detach(),
                   "pos_node_knn_indices": parts[2 * p][1], "anc_node_knn_indices": parts[2 * p + 1][1],
                   "pos_node_knn_masks": parts[2 * p][2], "anc_node_knn_masks": parts[2 * p + 1][2],
                   "pos_node_masks": parts[2 * p][0], "anc_node_masks": parts[2 * p + 1][0]} for p in range(P)]
        gt = get_node_correspondences_batched(labels, T, self.matching_radius)        # one native call (lcr_node_correspondences), no gradient
        sel = []
        for p in range(P):
            pi, ai, ov = self.coarse_target(*gt[p])                                    # host sync: the number of correspondences kept
            if pi.numel() == 0:
                raise RuntimeError("training forward: pair %d has no ground-truth node correspondence with an overlap above %g"
                                   % (p, self.coarse_target.overlap_threshold))
            sel.append((pi.long(), ai.long(), ov))
        q_off, pkp, akp, pkm, akm, ms = self._patch_transport_selected(P, pts_f, feats_f, off_m, knn_all, km_all, tab, sel)
        w, b = self.proj_node_overlap_score.weight, self.proj_node_overlap_score.bias
        for p in range(P):
            q = slice(q_off[p], q_off[p + 1])
            c = 2 * p
            pi, ai, ov = sel[p]
            score = torch.sigmoid(F.linear(fc[off_m[c]:off_m[c + 2]].contiguous(), w, b).view(-1)).clamp(0, 1)      # :146-147
            outs[p].update({
                "pos_points_c": nodes[off_m[c]:off_m[c + 1]], "anc_points_c": nodes[off_m[c + 1]:off_m[c + 2]],
                "pos_feats_c": fc[off_m[c]:off_m[c + 1]], "anc_feats_c": fc[off_m[c + 1]:off_m[c + 2]],
                "pos_points_f": pts_f[off_f[c]:off_f[c + 1]], "anc_points_f": pts_f[off_f[c + 1]:off_f[c + 2]],
                "pos_node_knn_indices": parts[c][1], "pos_node_knn_masks": parts[c][2], "anc_node_knn_indices": parts[c + 1][1],
                "anc_node_knn_masks": parts[c + 1][2], "pos_node_corr_indices": pi, "anc_node_corr_indices": ai, "node_corr_scores": ov,
                "pos_feats_f": feats_f[off_f[c]:off_f[c + 1]], "anc_feats_f": feats_f[off_f[c + 1]:off_f[c + 2]],
                "pos_node_corr_knn_points": pkp[q], "anc_node_corr_knn_points": akp[q], "pos_node_corr_knn_masks": pkm[q],
                "anc_node_corr_knn_masks": akm[q], "matching_scores": ms[q],
                "node_matching_scores": self._pair_node_scores(ns, p, m[c], m[c + 1], Mx, Nx),
                "pos_node_masks": parts[c][0], "anc_node_masks": parts[c + 1][0],
                "gt_node_corr_indices": gt[p][0], "gt_node_corr_overlaps": gt[p][1], "score": score})

    def _patch_transport_selected(self, P, pts_f, feats_f, off_m, knn_all, km_all, tab, sel):
        """The patch-level transport of the selected node correspondences sel[p] = (pos node indices, anc node indices, ...) of every pair in
        one call over the stack's point features (differentiable in feats_f and the patch-level alpha) -> (first patch of every pair q_off,
        the patch points of both sides [Q,K,3], their masks [Q,K], log scores [Q,K+1,K+1])."""
        n_all = pts_f.shape[0]
        q_off = [0]
        for pi, _, _ in sel:
            q_off.append(q_off[-1] + pi.numel())
        # patch point indices of the selected nodes as rows of the WHOLE stack (pad = n_all), every pair and side in one pass
        knn_g = torch.where(knn_all == tab[2][:, None], torch.full_like(knn_all, n_all), knn_all + tab[1][:, None])
        gi_rows = torch.cat([sel[p][0] + (off_m[2 * p] - off_m[0]) for p in range(P)])
        gj_rows = torch.cat([sel[p][1] + (off_m[2 * p + 1] - off_m[0]) for p in range(P)])
        pk_g, ak_g = knn_g[gi_rows].contiguous(), knn_g[gj_rows].contiguous()
        pkm, akm = km_all[gi_rows].contiguous(), km_all[gj_rows].contiguous()
        pkp, akp = F.gather_rows(pts_f, pk_g), F.gather_rows(pts_f, ak_g)
        with F.inverted_lists():
            ms = F.patch_log_optimal_transport(feats_f, pk_g, feats_f, ak_g, pkm, akm, self.optimal_transport.alpha,
                                               scale=1.0 / feats_f.shape[1] ** 0.5, iters=self.optimal_transport.num_iterations)
        return q_off, pkp, akp, pkm, akm, ms


def create_model(cfg=None):
    return LCRNet_Matching(cfg)
