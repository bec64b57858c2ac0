#!/usr/bin/env python
"""Vote_Encoder's and KPDecoder's forward + backward (lcr_kpconv_points_grad in csrc/kpconv_grad.hip, lcr_vote_shift_grad /
lcr_neighbor_mean_grad / lcr_upsample_concat_grad in csrc/pose_tail.hip behind the module tree) against their no-grad forwards, against torch
autograd on the same card through the guarded-sqrt restatement (tests/vote_grad_restatement.py) and oracle/torch_ref.kp_decoder, and
lcr_kpconv_points_grad against lcr_kpconv_aggregate and lcr_kpconv_aggregate_grad at the three encoder6 shapes.

    python tools/vote_encoder_grad_bench.py [--pairs 1 16] [--steps 10] [--warmup 3] [--out FILE]

The batch: 2 x pairs synthetic scans (lcrnet_amd.synthetic, seeds 0 ...), voxelised at 0.3 m and collated by precompute_batch with the
reference neighbour limits: coarse clouds of ~860 nodes.  The coarse 256-wide features and the decoder's skip features are seeded random
tensors of the shapes the model hands over; seeded weights.  A sample is a device-synchronised wall clock around one call; reported is the
median of --steps samples after --warmup, with the smallest and largest.  One JSON line per block:
  vote_encoder  forward_ms   the eval-mode forward under no_grad
                train_ms     training-mode forward + backward() of seeded cotangents on feats_c, points_c and shifted_points_c
                torch_train_ms (one pair only)  the same through torch autograd of the restatement, index lists given
  decoder       the same three for KPDecoder (torch: oracle/torch_ref.kp_decoder; loss on the finest features)
  points_grad   per encoder6 block: lcr_kpconv_aggregate, lcr_kpconv_aggregate_grad, lcr_kpconv_points_grad (both outputs) and the ratios"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VOXEL, RADIUS, SIGMA, NUM_STAGES = 0.3, 1.275, 0.6, 4
LIMITS = [64, 65, 74, 80]
MAX_RANGE = 4.2


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


def seeded(module, dev):
    from lcrnet_amd.weights import seeded_state_dict
    module.load_state_dict(seeded_state_dict(module.state_dict(), 7351), strict=True)
    return module.to(dev)


def randn(shape, seed, dev):
    import torch
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def leaves(module):
    return {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and not k.endswith("kernel_points")) for k, v in module.state_dict().items()}


def vote_lists(m, feats, dd):
    """the index computations of Vote_Encoder.forward, once, for the torch side"""
    import torch
    from lcrnet_amd import functional as F
    from lcrnet_amd.modules.ops import radius_search
    with torch.no_grad():
        pts, lens = dd["points"][-1], dd["lengths"][-1]
        shifted = m.vote(pts, feats)
        keep, length = F.greedy_nms(shifted, lens, m.NMS_radius)
        knn = radius_search(shifted[keep.bool()].contiguous(), shifted, length, lens, 2.4, LIMITS[-1], check=False)
        centers = F.neighbor_mean(shifted, knn, shifted.shape[0])
        sub = radius_search(centers, pts, length, lens, RADIUS * 8, LIMITS[-2], check=False)
        nb = radius_search(centers, centers, length, length, RADIUS * 16, LIMITS[-1], check=False)
    return dict(length=length, knn=knn, sub=sub, nb=nb)


def bench_vote(pairs, dd, steps, warmup, dev, with_torch):
    import torch
    import vote_grad_restatement as V
    from lcrnet_amd.config import make_cfg
    from lcrnet_amd.model_family.LCRNet import Vote_Encoder
    m = seeded(Vote_Encoder(64, 15, RADIUS, SIGMA, 32, make_cfg()["Vote"], LIMITS), dev)
    vd = {"points": [dd["points"][-1]], "lengths": [dd["lengths"][-1]]}
    n = vd["points"][0].shape[0]
    feats = randn((n, 256), 1, dev).requires_grad_(True)
    with torch.no_grad():
        out = m.eval()(feats, vd, pairs=pairs)
    nodes = out["feats_c"].shape[0]
    cot = {"feats_c": randn((nodes, 512), 2, dev) / nodes, "points_c": randn((nodes, 3), 3, dev) / nodes, "shifted_points_c": randn((n, 3), 4, dev) / n}
    res = {"bench": "vote_encoder_grad_bench", "block": "vote_encoder", "pairs": pairs, "coarse_points": n, "nodes": nodes,
           "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup}

    def forward():
        with torch.no_grad():
            m(feats, vd, pairs=pairs)

    def train():
        feats.grad = None
        for p in m.parameters():
            p.grad = None
        o = m(feats, vd, pairs=pairs)
        sum((o[k] * cot[k]).sum() for k in cot).backward()

    m.eval()
    res["forward_ms"] = timed(forward, steps, warmup)
    m.train()
    res["train_ms"] = timed(train, steps, warmup)
    res["train_over_forward"] = res["train_ms"]["ms"] / res["forward_ms"]["ms"]
    if with_torch:
        lists = vote_lists(m, feats.detach(), vd)
        sd = leaves(m)
        f = feats.detach().clone().requires_grad_(True)

        def torch_step():
            f.grad = None
            for v in sd.values():
                v.grad = None
            o = V.vote_encoder(sd, f, vd["points"][0], vd["lengths"][0].cpu(), lists, MAX_RANGE, pairs)
            sum((o[k] * cot[k]).sum() for k in cot).backward()

        res["torch_train_ms"] = timed(torch_step, max(3, steps // 2), 1)
        res["torch_over_hip"] = res["torch_train_ms"]["ms"] / res["train_ms"]["ms"]
    return res, m, vote_lists(m, feats.detach(), vd)


def bench_decoder(pairs, dd, steps, warmup, dev, with_torch):
    import torch
    from lcrnet_amd.model_family.LCRNet import KPDecoder
    from oracle import torch_ref
    m = seeded(KPDecoder(64, 32), dev)
    widths = (128, 256, 512, 256)
    feats = [randn((dd["points"][i].shape[0], widths[i]), 10 + i, dev).requires_grad_(True) for i in range(4)]
    n1 = feats[0].shape[0]
    cot = randn((n1, 128), 20, dev) / n1
    res = {"bench": "vote_encoder_grad_bench", "block": "decoder", "pairs": pairs, "stage_points": [int(f.shape[0]) for f in feats], "steps": steps,
           "warmup": warmup}

    def forward():
        with torch.no_grad():
            m(feats, dd, pairs=pairs)

    def train():
        for t in feats + list(m.parameters()):
            t.grad = None
        (m(feats, dd, pairs=pairs)[0] * cot).sum().backward()

    m.eval()
    res["forward_ms"] = timed(forward, steps, warmup)
    m.train()
    res["train_ms"] = timed(train, steps, warmup)
    res["train_over_forward"] = res["train_ms"]["ms"] / res["forward_ms"]["ms"]
    if with_torch:                                           # one pair: torch_ref's GroupNorm spans the stack it is given
        sd = leaves(m)
        up = {"upsampling": [u.long() for u in dd["upsampling"]]}
        fs = [f.detach().clone().requires_grad_(True) for f in feats]

        def torch_step():
            for t in fs + list(sd.values()):
                t.grad = None
            (torch_ref.kp_decoder(sd, fs, up, 32, pfx="") * cot).sum().backward()

        res["torch_train_ms"] = timed(torch_step, max(3, steps // 2), 1)
        res["torch_over_hip"] = res["torch_train_ms"]["ms"] / res["train_ms"]["ms"]
    return res


def bench_points_grad(pairs, m, lists, dd, steps, warmup):
    import torch
    from lcrnet_amd import functional as F
    pts = dd["points"][-1]
    with torch.no_grad():
        centers = F.neighbor_mean(m.vote(pts, randn((pts.shape[0], 256), 1, pts.device)), lists["knn"], pts.shape[0])
    rows = []
    for name, s, idx in (("encoder6_1", pts, lists["sub"]), ("encoder6_2", centers, lists["nb"]), ("encoder6_3", centers, lists["nb"])):
        conv = getattr(m, name).KPConv
        C, q = conv.in_channels, centers
        M, H, Ns = idx.shape[0], idx.shape[1], s.shape[0]
        f, dA = randn((Ns, C), 30, q.device), randn((M, 15 * C), 31, q.device)
        pos, kp = F.row_positive(f), conv.kernel_points_host()
        inv = F.neighbor_transpose(idx, Ns)
        row = {"block": name, "M": M, "Ns": Ns, "H": H, "C": C, "edges": int(inv[0][-1])}
        row["aggregate_ms"] = timed(lambda: F.kpconv_aggregate(f, pos, q, s, idx, kp, conv.sigma), steps, warmup)
        row["aggregate_grad_ms"] = timed(lambda: F.kpconv_aggregate_grad(dA, q, s, inv, H, kp, conv.sigma), steps, warmup)
        row["points_grad_ms"] = timed(lambda: F.kpconv_points_grad(dA, f, q, s, idx, kp, conv.sigma, inv), steps, warmup)
        row["points_grad_over_aggregate"] = row["points_grad_ms"]["ms"] / row["aggregate_ms"]["ms"]
        row["points_grad_over_aggregate_grad"] = row["points_grad_ms"]["ms"] / row["aggregate_grad_ms"]["ms"]
        rows.append(row)
    return {"bench": "vote_encoder_grad_bench", "block": "points_grad", "pairs": pairs, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool needs a GPU"
    dev = torch.device("cuda:0")
    lines = []
    for pairs in args.pairs:
        dd = collate(2 * pairs, dev)
        res, m, lists = bench_vote(pairs, dd, args.steps, args.warmup, dev, with_torch=pairs == 1)
        lines.append(res)
        lines.append(bench_points_grad(pairs, m, lists, dd, args.steps, args.warmup))
        lines.append(bench_decoder(pairs, dd, args.steps, args.warmup, dev, with_torch=pairs == 1))
        del dd, m, lists
        torch.cuda.empty_cache()
    for line in lines:
        print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
