"""Ground-truth node correspondences for the registration harness (modules/registration/matching.py:252-349 in the reference):
which (ref node, src node) patch pairs overlap under the ground-truth transform, and by how much.  Evaluation metadata of
`LCRNet_Matching.forward` (LCRNet_Matching.py:189-204) — label generation, not part of the timed path; device tensors in, device
tensors out, patch pairs processed in bounded chunks (the reference materialises all (B, K, K) distance blocks at once)."""
import torch


def _apply(points, transform):
    return points @ transform[:3, :3].t() + transform[:3, 3]


def _sq_dist(x, y):
    """|x|^2 - 2 x.y + |y|^2 clamped at 1e-12 — the reference's formula (ops/pairwise_distance.py:3-33), kept so that the labels
    agree with it at the radius threshold."""
    xy = x @ y.transpose(-1, -2)
    return ((x * x).sum(-1).unsqueeze(-1) - 2 * xy + (y * y).sum(-1).unsqueeze(-2)).clamp(min=1e-12)


@torch.no_grad()
def get_node_correspondences(ref_nodes, src_nodes, ref_knn_points, src_knn_points, transform, pos_radius, ref_masks=None, src_masks=None,
                             ref_knn_masks=None, src_knn_masks=None, chunk=2048):
    """-> corr_indices i64 (C, 2), corr_overlaps f32 (C,): node pairs whose patches share at least one point pair closer than
    `pos_radius` after `transform` is applied to the source side; overlap = mean of the two sides' fractions of covered points."""
    dev = ref_nodes.device
    M, N, K = ref_nodes.shape[0], src_nodes.shape[0], ref_knn_points.shape[1]
    src_nodes = _apply(src_nodes, transform)
    src_knn_points = _apply(src_knn_points.reshape(-1, 3), transform).reshape(N, -1, 3)
    ones = lambda *s: torch.ones(s, dtype=torch.bool, device=dev)
    ref_masks = ones(M) if ref_masks is None else ref_masks
    src_masks = ones(N) if src_masks is None else src_masks
    ref_knn_masks = ones(M, K) if ref_knn_masks is None else ref_knn_masks
    src_knn_masks = ones(N, src_knn_points.shape[1]) if src_knn_masks is None else src_knn_masks
    # patches whose enclosing spheres (+ radius) do not touch cannot overlap
    ref_r = torch.linalg.norm(ref_knn_points - ref_nodes[:, None], dim=-1).masked_fill(~ref_knn_masks, 0.0).max(1)[0]
    src_r = torch.linalg.norm(src_knn_points - src_nodes[:, None], dim=-1).masked_fill(~src_knn_masks, 0.0).max(1)[0]
    centre = torch.sqrt(_sq_dist(ref_nodes, src_nodes))
    touch = (ref_r[:, None] + src_r[None, :] + pos_radius - centre > 0) & ref_masks[:, None] & src_masks[None, :]
    ri, si = torch.nonzero(touch, as_tuple=True)
    overlaps = torch.empty(ri.shape[0], dtype=torch.float32, device=dev)
    for a in range(0, ri.shape[0], chunk):
        r, s = ri[a:a + chunk], si[a:a + chunk]
        rm, sm = ref_knn_masks[r], src_knn_masks[s]
        d = _sq_dist(ref_knn_points[r], src_knn_points[s]).masked_fill(~(rm[:, :, None] & sm[:, None, :]), 1e12)
        near = d < pos_radius ** 2
        ref_cov = near.any(-1).sum(-1).float() / rm.sum(-1).float()
        src_cov = near.any(-2).sum(-1).float() / sm.sum(-1).float()
        overlaps[a:a + chunk] = (ref_cov + src_cov) / 2
    keep = overlaps > 0
    return torch.stack([ri[keep], si[keep]], dim=1), overlaps[keep]


@torch.no_grad()
def get_node_correspondences_batched(outs, transforms, pos_radius=0.45):
    """The labels of every pair of a `forward_pairs` call in ONE native call (functional.node_correspondences; include/lcr_hip.h,
    lcr_node_correspondences): `outs` is the list of dicts `LCRNet.forward_pairs` returns (pos/anc_points_f, pos/anc_points_c,
    pos/anc_node_knn_indices, pos/anc_node_knn_masks and, when present, pos/anc_node_masks), `transforms` (P, 4, 4) or a list of
    (4, 4), anchor onto positive.  Stores gt_node_corr_indices i64 (C, 2) and gt_node_corr_overlaps f32 (C,) in each dict (what
    io_formats.save_registration writes) and returns them as a list of pairs.  More than 32 pairs go in slices of 32.
    Unlike `get_node_correspondences` above, nearness is decided on direct coordinate differences: the labels are a
    pure function of the inputs.  A dict without node masks (the plain LCRNet drops them) uses "the node has a valid patch point", which
    is what the partition's own node mask says."""
    from ... import functional as F
    outs = list(outs)
    T = torch.stack([torch.as_tensor(t) for t in transforms]) if isinstance(transforms, (list, tuple)) else transforms
    T = T.detach().reshape(-1, 4, 4)
    if T.shape[0] != len(outs):
        raise RuntimeError("one transform per pair: got %d for %d pairs" % (T.shape[0], len(outs)))
    result = []
    for g0 in range(0, len(outs), 32):
        group = outs[g0:g0 + 32]
        dev = group[0]["pos_points_f"].device
        pts, nodes, knn, km, nm, po, mo = [], [], [], [], [], [0], [0]
        for o in group:
            for side in ("pos", "anc"):
                k = o[side + "_node_knn_indices"]
                m = o[side + "_node_knn_masks"]
                pts.append(o[side + "_points_f"])
                nodes.append(o[side + "_points_c"])
                knn.append(k)
                km.append(m)
                nm.append(o[side + "_node_masks"] if side + "_node_masks" in o else m.bool().any(1))
                po.append(po[-1] + pts[-1].shape[0])
                mo.append(mo[-1] + k.shape[0])
        corr, ov, start = F.node_correspondences(torch.cat(pts).float(), po, torch.cat(nodes).float(), mo, torch.cat(knn), torch.cat(km),
                                                 torch.cat(nm), T[g0:g0 + 32].to(dev).float().contiguous(), pos_radius)
        s = start.tolist()
        for p, o in enumerate(group):
            o["gt_node_corr_indices"], o["gt_node_corr_overlaps"] = corr[s[p]:s[p + 1]], ov[s[p]:s[p + 1]]
            result.append((o["gt_node_corr_indices"], o["gt_node_corr_overlaps"]))
    return result
