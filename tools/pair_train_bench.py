#!/usr/bin/env python
"""One training step of the pair model — LCRNet_Matching.train() forward + OverallLoss_new + backward + fused Adan — against the eval forward
and against the same step with the patch scores on the torch path (functional.PATCH_SCORES_FUSED off = LCR_PATCH_SCORES_FUSED=0: gather,
torch.bmm and index_put atomics, what the step ran before lcr_patch_scores_grad), and lcr_patch_scores_grad against lcr_patch_scores and
against that torch path alone.

    python tools/pair_train_bench.py [--pairs 1 16] [--patches 128 2048] [--steps 10] [--warmup 3] [--out FILE]

The batch: `pairs` registration pairs, each a synthetic scan (lcrnet_amd.synthetic, seeds 0 ...) and the same scan under a known motion
(6 degrees about z, 1.0 / 0.5 / 0 m), voxelised at 0.3 m and collated by precompute_batch with the reference neighbour limits; seeded weights;
num_targets = 128.  A sample is a device-synchronised wall clock around one call.  The forms that are compared are ALTERNATED sample by
sample (fused, torch, fused, ...), so drift of the clock hits them alike; reported is the median of --steps samples after --warmup with the
smallest and largest.  One JSON line per block:
  step          eval_forward_ms, train_step_ms (fused), train_step_torch_ms, torch_over_fused, patches per call
  patch_scores  per P (C = 128, 40 000 feature rows, ~10 % masked slots): forward_ms (lcr_patch_scores), grad_ms (lcr_patch_scores_grad, lists
                built), lists_ms (the two lcr_neighbor_transpose calls), torch_forward_ms / torch_backward_ms (cat + index + bmm and its
                autograd backward to both feature tensors), and the ratios"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOXEL, RADIUS, NUM_STAGES = 0.3, 1.275, 4
LIMITS = [64, 65, 74, 80]


def timed_alternated(fns, steps, warmup):
    """{name: {"ms": median, "min_max": [...]}} with the functions called in turn inside every sample round"""
    import torch
    ts = {k: [] for k in fns}
    for r in range(warmup + steps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= warmup:
                ts[k].append((time.perf_counter() - t0) * 1e3)
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = {"ms": v[len(v) // 2], "min_max": [v[0], v[-1]]}
    return out


def collate(pairs, dev):
    import numpy as np
    import torch
    import lcrnet_amd.synthetic as synthetic
    from lcrnet_amd.data import precompute_batch, voxelize_raw_scans
    a = math.radians(6.0)
    R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    t = np.array([1.0, 0.5, 0.0])
    scans = []
    for i in range(pairs):
        pos = synthetic.synthetic_scan(i).astype(np.float64)
        scans += [pos.astype(np.float32), ((pos - t) @ R).astype(np.float32)]           # anc = R^T (pos - t): T maps anc onto pos
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    raw = torch.from_numpy(np.concatenate(scans)).to(dev)
    pts, lens_dev, _ = voxelize_raw_scans(raw, torch.tensor([len(s) for s in scans], device=dev), VOXEL)
    dd = precompute_batch(pts.contiguous(), lens_dev, NUM_STAGES, VOXEL, RADIUS, LIMITS)
    if pairs == 1:
        dd.pop("segment_lengths", None)
    dd["features"] = torch.ones(dd["points"][0].shape[0], 1, device=dev)
    dd["transform"] = torch.from_numpy(T).to(dev)[None].repeat(pairs, 1, 1)
    return dd


def bench_step(pairs, steps, warmup, dev):
    import torch
    from lcrnet_amd import functional as F
    from lcrnet_amd.adan import Adan
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.losses import OverallLoss_new
    from lcrnet_amd.model_family.LCRNet_Matching import LCRNet_Matching
    from lcrnet_amd.weights import seeded_state_dict
    cfg = make_cfg()
    model = LCRNet_Matching(cfg)
    model.load_state_dict(seeded_state_dict(model.state_dict(), 7351), strict=True)
    model = model.to(dev)
    dd = collate(pairs, dev)
    crit = OverallLoss_new(cfg)
    opt = Adan(model.parameters(), lr=1e-6, fused=True)
    info = {}

    def forward():
        model.eval()
        with torch.no_grad():
            model.forward_pairs(dd)

    def step(fused):
        def run():
            F.PATCH_SCORES_FUSED[0] = fused
            try:
                model.train()
                model.coarse_target.reseed()
                outs = model.forward_pairs(dd)
                info["patches"] = sum(o["matching_scores"].shape[0] for o in outs)
                loss = sum(ld["loss"] for ld in crit(outs, dd))
                opt.zero_grad()
                loss.backward()
                opt.step()
                info["loss"] = loss.detach()
            finally:
                F.PATCH_SCORES_FUSED[0] = True
        return run

    r = timed_alternated({"eval_forward_ms": forward, "train_step_ms": step(True), "train_step_torch_ms": step(False)}, steps, warmup)
    res = {"bench": "pair_train_bench", "block": "step", "pairs": pairs, "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup,
           "fine_points": int(dd["points"][0].shape[0]), "patches": info["patches"], "last_loss": float(info["loss"])}
    res.update(r)
    res["train_over_eval"] = r["train_step_ms"]["ms"] / r["eval_forward_ms"]["ms"]
    res["torch_over_fused"] = r["train_step_torch_ms"]["ms"] / r["train_step_ms"]["ms"]
    return res


def bench_patch_scores(P, steps, warmup, dev, C=128, N=40000, K=128):
    import torch
    from lcrnet_amd import functional as F
    g = torch.Generator().manual_seed(P)
    f = torch.randn(N, C, generator=g).to(dev)
    ia, ib = torch.randint(0, N, (P, K), generator=g), torch.randint(0, N, (P, K), generator=g)
    ma, mb = torch.rand(P, K, generator=g) > 0.1, torch.rand(P, K, generator=g) > 0.1
    ia[~ma], ib[~mb] = N, N
    ia, ib, ma8, mb8 = ia.to(dev), ib.to(dev), ma.to(torch.uint8).to(dev), mb.to(torch.uint8).to(dev)
    dS = torch.randn(P, K + 1, K + 1, generator=g).to(dev)
    alpha = torch.tensor(1.0, device=dev)
    scale = 1.0 / C ** 0.5
    inv = (F.neighbor_transpose(ia, N), F.neighbor_transpose(ib, N))
    fa, fb = f.clone().requires_grad_(True), f.clone().requires_grad_(True)
    cot = dS[:, :K, :K].contiguous()
    keep = {}

    def torch_forward():
        pa = torch.cat([fa, fa.new_zeros(1, C)])[ia]
        pb = torch.cat([fb, fb.new_zeros(1, C)])[ib]
        keep["raw"] = torch.bmm(pa, pb.transpose(1, 2))

    def torch_backward():
        torch.autograd.grad(keep["raw"], (fa, fb), cot)

    r = timed_alternated({
        "forward_ms": lambda: F._patch_scores(f, f, ia, ib, ma8, mb8, alpha, scale, 1e12),
        "grad_ms": lambda: F.patch_scores_grad(dS, f, f, ia, ib, ma8, mb8, scale, inv[0], inv[1]),
        "lists_ms": lambda: (F.neighbor_transpose(ia, N), F.neighbor_transpose(ib, N)),
        "torch_forward_ms": torch_forward,
        "torch_backward_ms": torch_backward}, steps, warmup)
    res = {"bench": "pair_train_bench", "block": "patch_scores", "P": P, "C": C, "rows": N, "steps": steps, "warmup": warmup}
    res.update(r)
    res["grad_over_forward"] = r["grad_ms"]["ms"] / r["forward_ms"]["ms"]
    res["torch_backward_over_grad"] = r["torch_backward_ms"]["ms"] / r["grad_ms"]["ms"]
    res["torch_backward_over_grad_and_lists"] = r["torch_backward_ms"]["ms"] / (r["grad_ms"]["ms"] + r["lists_ms"]["ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="*", default=[1, 16])
    ap.add_argument("--patches", type=int, nargs="*", default=[128, 2048])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool needs a GPU"
    dev = torch.device("cuda:0")
    lines = []
    for P in args.patches:
        lines.append(bench_patch_scores(P, args.steps, args.warmup, dev))
        print(json.dumps(lines[-1]), flush=True)
    for pairs in args.pairs:
        lines.append(bench_step(pairs, args.steps, args.warmup, dev))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
