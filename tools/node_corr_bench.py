#!/usr/bin/env python
"""Ground-truth node correspondences (csrc/node_corr.hip): the labelled evaluation end to end, and the native call against the torch form.

    python tools/node_corr_bench.py [--pairs 4] [--steps 20] [--warmup 3] [--batch 16] [--out DIR]

1. End to end: --pairs synthetic planted-motion pairs (a lcrnet_amd.synthetic scan voxelised at 0.3 m; the anchor is a random 88 % of it
   moved by the inverse of a planted motion, 3 degrees about z and (1.6, -0.9, 0.12) m, with 5 mm noise) go through PairPipeline with seeded weights,
   are labelled by ONE call of modules.registration.get_node_correspondences_batched, written with io_formats.save_registration and read back
   by tools/registration_eval.py, whose Coarse Matching line now has its values.  Seeded weights: the numbers say that the path runs, not
   how good a trained model is.
2. Timing at the demo pair's size (tests/golden/matching_golden.npz: 350 x 331 nodes, K = 128, scans 003854 / 000958): the native call
   for P = 1 and P = --batch copies of the pair against the torch form `get_node_correspondences` run pair by pair on the same tensors,
   gathers through the padded cloud included, as LCRNet_Matching.forward_pairs does.  Device-synchronised wall clock around whole calls
   after warm-up, median of --steps; `native_launches_ms` is the launch sequence alone on pre-allocated buffers, `native_ms` the Python
   entry with its allocation, host synchronisation and slicing.
One JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMITS = [74, 68, 70, 67]


def planted_pairs(n, dev):
    import lcrnet_amd.synthetic as synthetic
    from lcrnet_amd.data import voxelize_raw_scans
    a = np.deg2rad(3.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    T[:3, 3] = [1.6, -0.9, 0.12]
    work = []
    for i in range(n):
        raw = synthetic.synthetic_scan(40 + i)
        pos, _, _ = voxelize_raw_scans(torch.from_numpy(raw).to(dev), torch.tensor([len(raw)], device=dev), 0.3)
        rng = np.random.default_rng(i)
        p = pos.cpu().numpy().astype(np.float64)
        keep = rng.random(len(p)) < 0.88
        anc = ((p[keep] - T[:3, 3]) @ T[:3, :3] + rng.normal(scale=0.005, size=(int(keep.sum()), 3))).astype(np.float32)      # T maps anc onto pos
        anc = torch.from_numpy(anc).to(dev)
        work.append((torch.cat([pos.contiguous(), anc]), torch.tensor([len(pos), len(anc)], dtype=torch.int64, device=dev)))
    return work, T


def end_to_end(n_pairs, out_dir, dev):
    import registration_eval
    from lcrnet_amd import io_formats as io
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family import LCRNet
    from lcrnet_amd.modules.registration import get_node_correspondences_batched
    from lcrnet_amd.pipeline import PairPipeline
    from lcrnet_amd.weights import seeded_state_dict
    cfg = make_cfg()
    cfg["neighbor_limits"] = LIMITS
    m = LCRNet(cfg).eval()
    m.load_state_dict(seeded_state_dict(m.state_dict(), 7351), strict=True)
    m = m.to(dev)
    work, T = planted_pairs(n_pairs, dev)
    Tt = torch.from_numpy(T.astype(np.float32))
    with PairPipeline(m, 0.3, 1.275, 4, LIMITS, workers=1, pairs_per_call=min(16, max(2, n_pairs))) as pipe:
        outs = list(pipe.run(work))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        get_node_correspondences_batched(outs, [Tt] * len(outs), 0.45)
        torch.cuda.synchronize(dev)
        label_ms = (time.perf_counter() - t0) * 1e3
        labels = [int(o["gt_node_corr_indices"].shape[0]) for o in outs]
        nodes = [(int(o["pos_points_c"].shape[0]), int(o["anc_points_c"].shape[0])) for o in outs]
        for i, o in enumerate(outs):
            io.save_registration(out_dir, 0, 100 + i, 200 + i, o, T)
    res = registration_eval.main([out_dir])
    return {"pairs": n_pairs, "nodes": nodes, "labels_per_pair": labels, "label_call_ms": label_ms, "coarse_matching": res.get("coarse_matching"),
            "fine_matching": res["fine_matching"], "registration": res["registration"]}


def median_ms(fn, steps, warmup, dev):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize(dev)
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def timing(P, steps, warmup, dev):
    import node_corr_restatement as R
    from conftest import GOLDEN, load_scan
    from lcrnet_amd import functional as F
    from lcrnet_amd.modules.registration import get_node_correspondences
    gold = np.load(os.path.join(GOLDEN, "matching_golden.npz"))
    c = R.golden_case(gold, load_scan("003854"), load_scan("000958"))
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    po = np.concatenate([[0], np.cumsum(np.tile(np.diff(c["point_off"]), P))])
    mo = np.concatenate([[0], np.cumsum(np.tile(np.diff(c["node_off"]), P))])
    rep = lambda k: t(np.concatenate([c[k]] * P))
    pts, nodes, knn, km, nm, T = rep("points"), rep("nodes"), rep("knn"), rep("knn_mask"), rep("node_mask"), rep("transforms")
    native = lambda: F.node_correspondences(pts, po, nodes, mo, knn, km, nm, T, 0.45)
    corr, ov, start = native()
    bufs = F.node_correspondences_raw(pts, po, nodes, mo, knn, km, nm, T, 0.45)
    ws = torch.empty(F.node_correspondences_ws_bytes(po, mo, c["K"]), dtype=torch.uint8, device=dev)
    launches = lambda: F.node_correspondences_raw(pts, po, nodes, mo, knn, km, nm, T, 0.45, ws=ws, corr=bufs[0], overlap=bufs[1], start=bufs[2],
                                                  status=bufs[3])
    n0, n1 = len(load_scan("003854")), len(load_scan("000958"))
    pos_f, anc_f = t(c["points"][:n0]), t(c["points"][n0:])
    M = int(c["node_off"][1])
    pos_c, anc_c = t(c["nodes"][:M]), t(c["nodes"][M:])
    kp, ka, kmp, kma = t(c["knn"][:M]), t(c["knn"][M:]), t(c["knn_mask"][:M]).bool(), t(c["knn_mask"][M:]).bool()
    nmp, nma, T1 = t(c["node_mask"][:M]).bool(), t(c["node_mask"][M:]).bool(), t(c["transforms"][0])
    pad = lambda x: torch.cat([x, torch.zeros_like(x[:1])], 0)

    def torch_form():
        for _ in range(P):
            gi, go = get_node_correspondences(pos_c, anc_c, pad(pos_f)[kp.clamp(max=n0)], pad(anc_f)[ka.clamp(max=n1)], T1, 0.45, nmp, nma, kmp, kma)
        return gi, go

    gi, go = torch_form()
    s = start.tolist()
    same_rows = bool(torch.equal(corr[s[P - 1]:s[P]], gi))
    nat, nat_min = median_ms(native, steps, warmup, dev)
    lau, lau_min = median_ms(launches, steps, warmup, dev)
    tor, tor_min = median_ms(torch_form, max(3, steps // 4), 1, dev)
    return {"P": P, "rows_per_pair": s[1], "rows_equal_torch_form": same_rows,
            "overlaps_differ_from_torch_form": int((ov[s[P - 1]:s[P]] - go).abs().gt(1e-6).sum()) if same_rows else None,
            "native_ms": nat, "native_min_ms": nat_min, "native_launches_ms": lau, "native_launches_min_ms": lau_min, "torch_ms": tor,
            "torch_min_ms": tor_min}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--pairs", type=int, default=4)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--batch", type=int, default=16)
    p.add_argument("--out", default=None, help="directory for the pair files (default: a temporary one)")
    args = p.parse_args(argv)
    dev = torch.device("cuda", torch.cuda.current_device())
    out = {"timing": [timing(1, args.steps, args.warmup, dev), timing(args.batch, args.steps, args.warmup, dev)]}
    if args.pairs > 0:
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            out["end_to_end"] = end_to_end(args.pairs, args.out, dev)
        else:
            with tempfile.TemporaryDirectory() as d:
                out["end_to_end"] = end_to_end(args.pairs, d, dev)
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
