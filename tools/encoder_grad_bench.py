#!/usr/bin/env python
"""The KPEncoder's forward + backward (csrc/kpconv_grad.hip, csrc/groupnorm_grad.hip behind the module tree) against its native no-grad
forward, against torch autograd through oracle/torch_ref.kp_encoder on the same card, and lcr_kpconv_aggregate_grad against
lcr_kpconv_aggregate at every stage's shape.

    python tools/encoder_grad_bench.py [--scans 8] [--steps 10] [--warmup 3] [--out FILE]

The batch is bench.py's: --scans synthetic scans (seeds 0 ...), voxelised at 0.3 m, collated by precompute_batch with the reference neighbour
limits and per-scan GroupNorm segments; seeded weights.  A sample is a device-synchronised wall clock around one call; reported is the median
of --steps samples after --warmup, with the smallest and largest.  One JSON line per block:
  encoder     forward_ms      the native one-call forward under no_grad
              train_ms        forward through the module tree + backward() of a seeded scalar on the coarse features to every parameter
              lists_ms        the seven lcr_neighbor_transpose calls of a pass (part of train_ms)
  torch1      the same two at ONE scan, and torch autograd (forward + backward) through oracle/torch_ref.kp_encoder on the device
  aggregate   per encoder block with C_in > 1: lcr_kpconv_aggregate, lcr_kpconv_aggregate_grad, their ratio, and the in-degrees of the
              inverted list (median, maximum): the load balance of the wavefront-per-support gather"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VOXEL, RADIUS, SIGMA, NUM_STAGES = 0.3, 1.275, 0.6, 4
LIMITS = [64, 65, 74, 80]


def timed(fn, steps, warmup):
    import torch
    ts = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"ms": ts[len(ts) // 2], "min_max": [ts[0], ts[-1]]}


def collate(n_scans, dev):
    import numpy as np
    import torch
    import lcrnet_amd.synthetic as synthetic
    from lcrnet_amd.data import precompute_batch, voxelize_raw_scans
    scans = [synthetic.synthetic_scan(i) for i in range(n_scans)]
    raw = torch.from_numpy(np.concatenate(scans)).to(dev)
    pts, lens_dev, _ = voxelize_raw_scans(raw, torch.tensor([len(s) for s in scans], device=dev), VOXEL)
    return precompute_batch(pts.contiguous(), lens_dev, NUM_STAGES, VOXEL, RADIUS, LIMITS)


def encoder(dev):
    from lcrnet_amd.backbone4 import KPEncoder
    from lcrnet_amd.weights import seeded_state_dict
    enc = KPEncoder(1, 64, 15, RADIUS, SIGMA, 32)
    enc.load_state_dict(seeded_state_dict(enc.state_dict(), 7351), strict=True)
    return enc.to(dev)


def train_step(enc, feats, dd, target):
    import torch
    for p in enc.parameters():
        p.grad = None
    out = enc(feats, dd)[-1]
    (out * target).sum().backward()


def bench_encoder(n_scans, steps, warmup, dev, with_torch):
    import torch
    from lcrnet_amd import functional as F
    from oracle import torch_ref
    dd = collate(n_scans, dev)
    enc = encoder(dev)
    feats = torch.ones(dd["points"][0].shape[0], 1, device=dev)
    with torch.no_grad():
        coarse = enc(feats, dd)[-1]
    target = torch.randn(coarse.shape, generator=torch.Generator().manual_seed(1)).to(dev) / coarse.shape[0]
    res = {"bench": "encoder_grad_bench", "block": "torch1" if with_torch else "encoder", "scans": n_scans, "stage_points": [int(p.shape[0]) for p in dd["points"]],
           "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup}

    def forward():
        with torch.no_grad():
            enc(feats, dd)

    def lists():
        for i in range(4):
            F.neighbor_transpose(dd["neighbors"][i], dd["points"][i].shape[0])
        for i in range(3):
            F.neighbor_transpose(dd["subsampling"][i], dd["points"][i].shape[0])

    res["forward_ms"] = timed(forward, steps, warmup)
    res["train_ms"] = timed(lambda: train_step(enc, feats, dd, target), steps, warmup)
    res["lists_ms"] = timed(lists, steps, warmup)
    res["train_over_forward"] = res["train_ms"]["ms"] / res["forward_ms"]["ms"]
    if with_torch:
        sd = {"encoder." + k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("kernel_points")) for k, v in enc.state_dict().items()}
        ref = {k: [t.long() if not t.dtype.is_floating_point else t for t in dd[k]] for k in ("points", "neighbors", "subsampling")}
        seg = [[int(v) for v in l] for l in dd["lengths_host"]]

        def torch_step():
            for v in sd.values():
                v.grad = None
            out = torch_ref.kp_encoder(sd, feats, ref, init_sigma=SIGMA, groups=32, segment_lengths=seg)[-1]
            (out * target).sum().backward()

        res["torch_train_ms"] = timed(torch_step, max(3, steps // 2), 1)
        res["torch_over_hip"] = res["torch_train_ms"]["ms"] / res["train_ms"]["ms"]
    return res, dd, enc


def bench_aggregate(dd, enc, steps, warmup):
    import torch
    from lcrnet_amd import functional as F
    from oracle.torch_ref import ENCODER_PLAN
    rows = []
    for name, qs, ss, kind, mult, strided in ENCODER_PLAN:
        block = getattr(enc, name)
        C = block.KPConv.in_channels
        if C == 1:
            continue
        idx = dd[kind][ss if kind == "subsampling" else qs]
        q, s = dd["points"][qs], dd["points"][ss]
        M, H, Ns = idx.shape[0], idx.shape[1], s.shape[0]
        gen = torch.Generator().manual_seed(qs * 10 + ss)
        f = torch.randn(Ns, C, generator=gen).to(q.device)
        dA = torch.randn(M, 15 * C, generator=gen).to(q.device)
        pos = F.row_positive(f)
        kp = block.KPConv.kernel_points_host()
        inv = F.neighbor_transpose(idx, Ns)
        deg = (inv[0][1:] - inv[0][:-1]).float()
        row = {"block": name, "M": M, "Ns": Ns, "H": H, "C": C, "in_degree_median": float(deg.median()), "in_degree_max": float(deg.max()),
               "edges": int(inv[0][-1])}
        row["aggregate_ms"] = timed(lambda: F.kpconv_aggregate(f, pos, q, s, idx, kp, block.KPConv.sigma), steps, warmup)
        row["aggregate_grad_ms"] = timed(lambda: F.kpconv_aggregate_grad(dA, q, s, inv, H, kp, block.KPConv.sigma), steps, warmup)
        row["grad_over_forward"] = row["aggregate_grad_ms"]["ms"] / row["aggregate_ms"]["ms"]
        # bytes the reverse moves at least: the dA blocks with a non-zero influence are not known here; the whole of dA is the upper bound
        row["dA_bytes"] = M * 15 * C * 4
        rows.append(row)
    return {"bench": "encoder_grad_bench", "block": "aggregate", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool needs a GPU"
    dev = torch.device("cuda:0")
    lines = []
    res, dd, enc = bench_encoder(args.scans, args.steps, args.warmup, dev, with_torch=False)
    lines.append(res)
    lines.append(bench_aggregate(dd, enc, args.steps, args.warmup))
    del dd, enc
    torch.cuda.empty_cache()
    lines.append(bench_encoder(1, args.steps, args.warmup, dev, with_torch=True)[0])
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
