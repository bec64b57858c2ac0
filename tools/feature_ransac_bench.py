#!/usr/bin/env python
"""Feature-matching RANSAC timings (csrc/feature_nn.hip, lcr_ransac_correspondences_ex); one JSON line.

    python tools/feature_ransac_bench.py [--n 12000] [--channels 256] [--pairs 16] [--iterations 50000] [--repeats 5] [--warmup 2]

Every figure is a device-synchronised wall clock around whole calls after warm-up; the sides of a comparison alternate inside every
repeat, and the median is reported with the minimum and maximum over the repeats next to it.
  feature_nn   n x n x channels for S = 1 and S = --pairs: the native exact nearest neighbour against what torch offers on the same GPU,
               `torch.cdist(q, d).argmin(1)` per pair and the `|q|^2 + |d|^2 - 2 q d^T` matmul form (neither is exact in its ties nor
               batch-invariant; both hold an n x n matrix per pair).  Peak allocator memory of each side, the rate in rounded fp32
               operations (3 per (i, j, channel)) and its share of the vector unit's non-fused issue rate (256 CUs x 4 SIMD x 32 lanes x
               2.4 GHz = 78.6 T/s).  There is no screening pass, hence no matrix-core rate and no fall-back rate to report.
  ransac       50 000 iterations over the feature correspondences of planted pairs (one per source point), ransac_n 3 and 4, S = 1 and
               S = --pairs: the checked entry (edge 0.9, distance 0.3 m) against the unchecked lcr_ransac_correspondences on the same rows,
               with the share of hypotheses each checker rejected.
  end_to_end   registration.ransac_from_feats_batched per pair at S = --pairs (both NN directions with the mutual filter)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

VALU_OPS_PER_S = 256 * 4 * 32 * 2.4e9


def alternate(sides, repeats, warmup):
    """{name: fn} -> {name: {median_ms, min_ms, max_ms, peak_mib}}; the sides run one after the other inside every repeat"""
    times = {k: [] for k in sides}
    peak = {k: 0 for k in sides}
    for r in range(warmup + repeats):
        for k, fn in sides.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r >= warmup:
                times[k].append(dt * 1e3)
                peak[k] = max(peak[k], torch.cuda.max_memory_allocated() - base)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "peak_mib": peak[k] / 2 ** 20}
            for k, v in times.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=12000)
    p.add_argument("--channels", type=int, default=256)
    p.add_argument("--pairs", type=int, default=16)
    p.add_argument("--iterations", type=int, default=50000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    args = p.parse_args()
    import feature_ransac_restatement as fr
    from lcrnet_amd import functional as F
    from lcrnet_amd.registration import ransac_from_feats_batched

    dev = torch.device("cuda:0")
    n, C, P = args.n, args.channels, args.pairs
    g = torch.Generator(device="cpu").manual_seed(0)
    out = {"n": n, "channels": C, "pairs": P, "iterations": args.iterations, "repeats": args.repeats, "warmup": args.warmup}

    # ---- feature NN
    q = torch.nn.functional.normalize(torch.randn(P * n, C, generator=g), dim=1).to(dev)
    d = torch.nn.functional.normalize(torch.randn(P * n, C, generator=g), dim=1).to(dev)
    out["feature_nn"] = {}
    for S in sorted({1, P}):
        st = torch.arange(0, S + 1, dtype=torch.int32, device=dev) * n
        qs, ds = q[:S * n], d[:S * n]

        def cdist():
            return [torch.cdist(qs[i * n:(i + 1) * n], ds[i * n:(i + 1) * n]).argmin(1) for i in range(S)]

        def matmul():
            r = []
            for i in range(S):
                a, b = qs[i * n:(i + 1) * n], ds[i * n:(i + 1) * n]
                r.append(((a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)).argmin(1))
            return r

        res = alternate({"native": lambda: F.feature_nn(qs, ds, st, st), "torch_cdist_argmin": cdist, "torch_matmul_argmin": matmul},
                        args.repeats, args.warmup)
        nn = F.feature_nn(qs, ds, st, st)[0]
        res["rows_where_torch_cdist_agrees"] = float((torch.cat(cdist()) == nn).float().mean())
        ops = 3.0 * S * n * n * C
        res["native_rounded_ops_per_s"] = ops / (res["native"]["median_ms"] * 1e-3)
        res["native_share_of_valu_issue_rate"] = res["native_rounded_ops_per_s"] / VALU_OPS_PER_S
        res["native_ms_per_pair"] = res["native"]["median_ms"] / S
        out["feature_nn"]["S=%d" % S] = res

    # ---- checked against unchecked RANSAC on the feature correspondences of planted pairs (the per-channel feature noise of the test
    # pairs, scaled to the channel count)
    items = [fr.planted_feature_pair(n, 0.35, 0.15 * (32.0 / C) ** 0.5, seed=500 + i, C=C) for i in range(P)]
    cat = lambda k, w: torch.from_numpy(np.concatenate([it[k] for it in items]).reshape(-1, w)).to(dev)
    sp, rp, sf, rf = cat(0, 3), cat(1, 3), cat(2, C), cat(3, C)
    out["ransac"] = {}
    for S in sorted({1, P}):
        st = torch.arange(0, S + 1, dtype=torch.int32, device=dev) * n
        nn = F.feature_nn(sf[:S * n], rf[:S * n], st, st)[0].long()
        src = sp[:S * n].contiguous()
        ref = torch.cat([rp[i * n:(i + 1) * n][nn[i * n:(i + 1) * n]] for i in range(S)]).contiguous()
        for k in (3, 4):
            res = alternate({"checked": lambda: F.ransac_correspondences_ex(src, ref, st, 0.3, k, args.iterations, 0, edge_similarity=0.9,
                                                                            checker_distance=0.3),
                             "unchecked": lambda: F.ransac_correspondences(src, ref, st, 0.3, k, args.iterations, 0)}, args.repeats, args.warmup)
            r = F.ransac_correspondences_ex(src, ref, st, 0.3, k, args.iterations, 0, edge_similarity=0.9, checker_distance=0.3, want_reject=True)
            rej = r[4].cpu().numpy()
            ok = sum(1 for i in range(S) if np.abs(r[0][i].cpu().numpy().astype(np.float64) - items[i][4]).max() < 0.05)
            res.update(rejected={"degenerate": float((rej == 1).mean()), "edge_length": float((rej == 2).mean()),
                                 "distance": float((rej == 3).mean())}, reach_scoring=float((rej == 0).mean()),
                       checked_over_unchecked=res["checked"]["median_ms"] / res["unchecked"]["median_ms"], planted_pairs_recovered=ok)
            out["ransac"]["S=%d,ransac_n=%d" % (S, k)] = res

    # ---- end to end, S = pairs
    lens = [n] * P
    out["end_to_end"] = {}
    for mutual in (False, True):
        res = alternate({"call": lambda: ransac_from_feats_batched(sp, rp, sf, rf, lens, lens, 0.3, 3, args.iterations, 0, mutual_filter=mutual)},
                        args.repeats, args.warmup)["call"]
        res["ms_per_pair"] = res["median_ms"] / P
        out["end_to_end"]["mutual_filter=%s" % mutual] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
