#!/usr/bin/env python
"""The native registration loss (lcrnet_amd.losses.OverallLoss_new, csrc/losses.hip) against the torch form on the same card.

    python tools/loss_bench.py [--steps 30] [--warmup 5] [--pairs 1 16] [--out FILE]

Workload per pair, the registration workload's shapes: 256 patch pairs of 128 x 128 points (matching_scores 256 x 129 x 129), 500 x 500
nodes (node_matching_scores 501 x 501 with ~1500 ground-truth correspondences), 25 000 fine points and 500 shifted nodes per cloud.
Synthetic tensors from a seed: the numbers say what the loss costs, not what a trained model's loss is.

The torch form is the definition (include/lcr_hip.h, tests/losses_restatement.py) written with dense fp32 torch ops on the device, pair by
pair as the reference's loop does: label masks and where() for the gap terms, full distance matrices by differences for the two distance
terms.  Both forms are timed forward (`fwd`) and forward + backward to the scores and the shifted nodes (`fwd_bwd`): device-synchronised
wall clock around whole calls, --warmup calls first, then the median of --steps calls, the two forms alternating.  The values of the two
forms are compared before anything is timed.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS, GAMMA, THR, CORRES = 0.45, 0.5, 0.1, 2.4
GRAD_KEYS = ("matching_scores", "node_matching_scores", "shifted_pos_points_c", "shifted_anc_points_c")


def make_pair(seed, dev, B=256, K=128, nodes=500, fine=25000):
    g = torch.Generator(device="cpu").manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    n = lambda *s: torch.randn(*s, generator=g)
    centre = (r(B, 1, 3) - 0.5) * torch.tensor([120.0, 120.0, 6.0])
    pp = centre + (r(B, K, 3) - 0.5) * 3.0
    qp = pp[:, torch.randperm(K, generator=g)] + n(B, K, 3) * 0.4
    pm, qm = torch.ones(B, K, dtype=torch.bool), torch.ones(B, K, dtype=torch.bool)
    pm[:, K - 12:], qm[:, K - 9:] = False, False
    pp, qp = pp * pm[..., None], qp * qm[..., None]
    ms = n(B, K + 1, K + 1) * 3 - 8
    ms[:, :K][~pm] = -1e12
    ms.transpose(1, 2)[:, :K][~qm] = -1e12
    nm_p, nm_a = torch.ones(nodes, dtype=torch.bool), torch.ones(nodes, dtype=torch.bool)
    nm_p[nodes - 7:], nm_a[nodes - 4:] = False, False
    ns = n(nodes + 1, nodes + 1) * 3 - 8
    ns[:nodes][~nm_p] = -1e12
    ns[:, :nodes][:, ~nm_a] = -1e12
    flat = torch.randperm(nodes * nodes, generator=g)[:3 * nodes]
    corr = torch.stack([flat // nodes, flat % nodes], 1)
    pos_f = (r(fine, 3) - 0.5) * torch.tensor([120.0, 120.0, 6.0])
    anc_f = (r(fine, 3) - 0.5) * torch.tensor([120.0, 120.0, 6.0])
    ori_pos = pos_f[torch.randperm(fine, generator=g)[:nodes]]
    ori_anc = torch.cat([ori_pos[:nodes // 2] + n(nodes // 2, 3) * 0.3, anc_f[torch.randperm(fine, generator=g)[:nodes - nodes // 2]]])
    o = {"matching_scores": ms, "pos_node_corr_knn_points": pp, "anc_node_corr_knn_points": qp, "pos_node_corr_knn_masks": pm,
         "anc_node_corr_knn_masks": qm, "node_matching_scores": ns, "gt_node_corr_indices": corr,
         "gt_node_corr_overlaps": r(len(corr)) * 0.99 + 0.005, "pos_node_masks": nm_p, "anc_node_masks": nm_a,
         "shifted_pos_points_c": ori_pos + n(nodes, 3) * 0.8, "shifted_anc_points_c": ori_anc + n(nodes, 3) * 0.8, "pos_points_f": pos_f,
         "anc_points_f": anc_f, "ori_pos_points_c": ori_pos, "ori_anc_points_c": ori_anc, "pos_points_c": ori_pos, "anc_points_c": ori_anc,
         "score": r(2 * nodes) * 0.96 + 0.02, "pos_emb": n(1, nodes, 64) * 2.5, "anc_emb": n(1, nodes, 64) * 2.5}
    return {k: v.to(dev) for k, v in o.items()}


# ---- the torch form ---------------------------------------------------------------------------------------------------------------------------
def d2_diff(p, q):
    d = p[..., :, None, :] - q[..., None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def direction(S, pos, neg):
    dust = pos.sum(2) == 0
    posf, negf = torch.cat([pos, dust[..., None]], 2), torch.cat([neg, ~dust[..., None]], 2)
    line = (-S * posf).sum(2) / posf.sum(2)
    keep = line.detach() != 1e12
    s = (torch.clamp(line[..., None] + S + GAMMA, min=0) * negf).sum(2)
    return torch.log(s[keep] + 1).mean()


def gap_form(S, pos, neg):
    return (direction(S[:, :-1, :], pos, neg) + direction(S[:, :, :-1].transpose(1, 2), pos.transpose(1, 2), neg.transpose(1, 2))) / 2


def torch_form(o, T):
    R, t = T[:3, :3], T[:3, 3]
    d2 = d2_diff(o["pos_node_corr_knn_points"], o["anc_node_corr_knn_points"] @ R.t() + t)
    both = o["pos_node_corr_knn_masks"][:, :, None] & o["anc_node_corr_knn_masks"][:, None, :]
    g = gap_form(o["matching_scores"], (d2 < RADIUS * RADIUS) & both, d2 > (2 * RADIUS) ** 2)
    ns = o["node_matching_scores"]
    ov = torch.zeros(ns.shape[0] - 1, ns.shape[1] - 1, device=ns.device)
    ov[o["gt_node_corr_indices"][:, 0], o["gt_node_corr_indices"][:, 1]] = o["gt_node_corr_overlaps"]
    c = gap_form(ns[None], ((ov > THR) & o["pos_node_masks"][:, None] & o["anc_node_masks"][None, :])[None], (ov == 0)[None])
    sp, sa = o["shifted_pos_points_c"], o["shifted_anc_points_c"] @ R.t() + t
    dm = torch.sqrt(d2_diff(sp, sa).clamp(min=1e-12))
    vp, va = o["mask"]
    v = dm.min(1)[0][vp].mean() + dm.min(0)[0][va].mean()
    near = lambda a, d: torch.sqrt(d2_diff(a, d).clamp(min=1e-12)).min(1)[0].mean()
    d = (near(sp, o["pos_points_f"]) + near(o["shifted_anc_points_c"], o["anc_points_f"])) / 2
    gt = torch.zeros(o["score"].shape[0], device=ns.device)
    gt[o["gt_node_corr_indices"][:, 0]] = 1.0
    gt[o["pos_points_c"].shape[0] + o["gt_node_corr_indices"][:, 1]] = 1.0
    w_neg = gt.sum() / gt.shape[0]
    n = (torch.where(gt >= 0.5, 1 - w_neg, w_neg) * torch.nn.functional.binary_cross_entropy(o["score"], gt, reduction="none")).mean()
    beyond = lambda e: torch.clamp(e.abs() - 3.1415926, min=0).mean()
    reg = (beyond(o["pos_emb"]) + beyond(o["anc_emb"])) / 2
    return {"c_loss": c, "g_loss": 5 * g, "reg_loss": reg, "v_loss": 0.25 * v, "d_loss": 0.25 * d, "n_loss": n,
            "loss": c + 5 * g + reg + 0.25 * (v + d) + n}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench needs a GPU: a timing without one says nothing")
    import lcrnet_amd.losses as L
    from lcrnet_amd.config import make_cfg
    dev = torch.device("cuda:0")
    native = L.OverallLoss_new(make_cfg())
    res = {"bench": "loss_bench", "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup, "cases": []}
    for P in a.pairs:
        outs = [make_pair(100 + p, dev) for p in range(P)]
        T = torch.eye(4, device=dev).repeat(P, 1, 1)
        for p, o in enumerate(outs):
            o["mask"] = L.vote_mask(o["ori_pos_points_c"], o["ori_anc_points_c"], T[p], CORRES)
        data = {"transform": T}

        def leaves(on):
            for o in outs:
                for k in GRAD_KEYS:
                    o[k].requires_grad_(on)
                    o[k].grad = None

        def run_native(bwd):
            r = native(outs, data)
            if bwd:
                sum(x["loss"] for x in r).backward()
            return r

        def run_torch(bwd):
            r = [torch_form(o, T[p]) for p, o in enumerate(outs)]
            if bwd:
                sum(x["loss"] for x in r).backward()
            return r

        leaves(False)
        with torch.no_grad():
            nv, tv = run_native(False), run_torch(False)
        worst = max(abs(float(x[k]) - float(y[k])) / max(1.0, abs(float(y[k]))) for x, y in zip(nv, tv) for k in x)
        case = {"pairs": P, "max_relative_difference_native_vs_torch": worst, "loss_pair0": float(nv[0]["loss"])}
        for name, bwd in (("fwd", False), ("fwd_bwd", True)):
            leaves(bwd)
            tn, tt = [], []
            ctx = torch.enable_grad() if bwd else torch.no_grad()
            with ctx:
                timed(lambda: run_native(bwd), 0, a.warmup)
                timed(lambda: run_torch(bwd), 0, a.warmup)
                for _ in range(a.steps):                             # alternate the two forms
                    leaves(bwd)
                    tn += timed(lambda: run_native(bwd), 1, 0)
                    leaves(bwd)
                    tt += timed(lambda: run_torch(bwd), 1, 0)
            case[name] = {"native_ms": float(np.median(tn)), "torch_ms": float(np.median(tt)), "ratio_torch_over_native": float(np.median(tt) / np.median(tn)),
                          "native_ms_min_max": [float(min(tn)), float(max(tn))], "torch_ms_min_max": [float(min(tt)), float(max(tt))]}
        res["cases"].append(case)
        del outs
        torch.cuda.empty_cache()
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
