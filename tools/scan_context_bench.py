#!/usr/bin/env python
"""Scan Context (csrc/scan_context.hip) timings; one JSON line per measurement, appended to --out when given.

    python tools/scan_context_bench.py [--sizes 512,4541] [--unique 8] [--candidates 10,50] [--sample 0.2] [--samples 5] [--out FILE.jsonl]

Measurements (device-synchronised wall clock around whole native calls after a warm-up; a sample repeats the call until --sample seconds have
passed, the median of --samples samples is reported):
  descriptor  one lcr_scan_context call over 64 synthetic 64-beam scans (--unique distinct ones, a rigid motion per scan);
  search      the exhaustive causal search (k = 50, exclude = 100, queries 101 .. C - 2) over C synthetic descriptors, with the fp32 work it
              does counted from the formula: per pair 2 * 64 * 64 * K flops issued on the MFMA (W padded to 64, K = R padded to a multiple
              of 4) of which 2 * W * W * R are the definition's, plus W * W additions of the diagonal walk, against the 90 TFLOP/s the fp32
              GEMM family records;
              the two-stage form (ring-key kNN through lcr_retrieval_topk, then lcr_scan_context_distance on the candidates) and its top-1
              recall against the exhaustive search;
              a dense torch form on the same card (einsum Gram matrices of a block of queries, a gather per shift) on a share of the
              queries, and the NumPy restatement of tests/scan_context_restatement.py on a few pairs, both scaled to the whole search."""
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

K, EXCLUDE, START = 50, 100, 101
PEAK_FP32_MFMA_TFLOPS = 90.0


def sample(fn, seconds, samples):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= seconds:
                break
        out.append(dt / n)
    return float(np.median(out)), [round(x * 1e3, 4) for x in out]


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def synthetic_descriptors(C, R, W, dev, seed=4541):
    """C related polar images: a street-like base image, per-frame occlusions and a per-frame column shift; every 97th frame revisits an
    earlier one with noise -> ScanContexts built by the restatement's fp32 rules on the device"""
    from lcrnet_amd.scan_context import ScanContexts
    g = torch.Generator(device="cpu").manual_seed(seed)
    base = torch.rand((8, R, W), generator=g) * 6.0
    desc = base[torch.randint(0, 8, (C,), generator=g)] * (torch.rand((C, R, W), generator=g) < 0.8) + torch.rand((C, R, W), generator=g)
    desc = desc * (torch.rand((C, 1, W), generator=g) < 0.95)
    for i in range(C):
        desc[i] = torch.roll(desc[i], int(torch.randint(0, W, (1,), generator=g)), 1)
    for i in range(150, C, 97):
        desc[i] = torch.roll(desc[i - 140], 7, 1) + 0.01 * torch.randn((R, W), generator=g)
    desc = desc.float().to(dev)
    n = desc.square().sum(1).sqrt()
    unit = torch.where(n[:, None, :] > 0, desc / n[:, None, :].clamp_min(1e-30), torch.zeros_like(desc))
    bits = (n > 0).to(torch.int64) << torch.arange(W, device=dev)[None, :]
    return ScanContexts(desc, desc.mean(2), unit.contiguous(), bits.sum(1))


def torch_dense(unit, mask_bits, q0, q1, exclude):
    """the same distances with library calls: G = einsum over rings, then for each shift a gathered diagonal; [q1 - q0, q1 - exclude] block"""
    W = unit.shape[2]
    nj = max(1, q1 - 1 - exclude)
    G = torch.einsum("qrj,crk->qcjk", unit[q0:q1], unit[:nj])                      # [Q, nj, W, W]
    V = mask_bits[q0:q1, None, :, None] & mask_bits[None, :nj, None, :]
    G = torch.where(V, G, torch.zeros_like(G))
    j = torch.arange(W, device=unit.device)
    best = None
    for s in range(W):
        col = (j + s) % W
        sums, c = G[:, :, j, col].sum(-1), V[:, :, j, col].sum(-1)
        d = torch.where(c > 0, 1.0 - sums / c.clamp_min(1), torch.ones_like(sums))
        best = d if best is None else torch.minimum(best, d)
    return best


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sizes", default="512,4541")
    p.add_argument("--unique", type=int, default=8)
    p.add_argument("--candidates", default="10,50")
    p.add_argument("--sample", type=float, default=0.2)
    p.add_argument("--samples", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import scan_context_restatement as R
    import lcrnet_amd.synthetic as synthetic
    from lcrnet_amd import functional as F
    from lcrnet_amd import scan_context as sc_mod
    dev = torch.device("cuda:0")
    date = time.strftime("%Y-%m-%d")
    Rn, W = F.SCAN_CONTEXT_PARAMS["R"], F.SCAN_CONTEXT_PARAMS["W"]

    base = [synthetic.synthetic_scan(1000 + u) for u in range(args.unique)]
    clouds = []
    for i in range(64):
        a = i * 2.39996
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]], np.float32)
        clouds.append(base[i % len(base)] @ Rz.T)
    pts = torch.from_numpy(np.concatenate(clouds)).to(dev)
    ln = [len(c) for c in clouds]
    t, all_t = sample(lambda: F.scan_context(pts, ln), args.sample, args.samples)
    emit({"measurement": "descriptor", "date": date, "clouds": 64, "points": int(sum(ln)), "ms_per_call": t * 1e3, "samples_ms": all_t,
          "scans_per_s": 64 / t, "gbytes_per_s_of_points": 12 * sum(ln) / t / 1e9}, args.out)

    for C in [int(x) for x in args.sizes.split(",")]:
        sc = synthetic_descriptors(C, Rn, W, dev)
        q0, q1 = START, C - 1
        pairs = int(sum(max(0, i - EXCLUDE) for i in range(q0, q1)))
        t, all_t = sample(lambda: sc_mod.scan_context_topk(sc, q0, q1, K, EXCLUDE), args.sample, args.samples)
        k4 = (Rn + 3) // 4 * 4
        issued, defined = pairs * 2.0 * 64 * 64 * k4, pairs * (2.0 * W * W * Rn + W * W)
        idx, dist, shift = sc_mod.scan_context_topk(sc, q0, q1, K, EXCLUDE)
        emit({"measurement": "search", "form": "exhaustive", "date": date, "frames": C, "pairs": pairs, "ms_per_call": t * 1e3, "samples_ms": all_t,
              "ns_per_pair": t / pairs * 1e9, "mfma_tflops_issued": issued / t / 1e12, "tflops_of_the_definition": defined / t / 1e12,
              "share_of_fp32_mfma_peak_issued": issued / t / 1e12 / PEAK_FP32_MFMA_TFLOPS,
              "share_of_fp32_mfma_peak_defined": defined / t / 1e12 / PEAK_FP32_MFMA_TFLOPS}, args.out)
        for n_cand in [int(x) for x in args.candidates.split(",")]:
            k2 = min(K, n_cand)
            t2, all_t2 = sample(lambda: sc_mod.two_stage_topk(sc, n_cand, k2, EXCLUDE, q0, q1), args.sample, args.samples)
            idx2 = sc_mod.two_stage_topk(sc, n_cand, k2, EXCLUDE, q0, q1)[0]
            emit({"measurement": "search", "form": "two-stage", "date": date, "frames": C, "candidates": n_cand, "ms_per_call": t2 * 1e3,
                  "samples_ms": all_t2, "top1_recall_against_exhaustive": float((idx2[:, 0] == idx[:, 0]).float().mean())}, args.out)
        # dense torch form on a block of 8 late queries (the [8, C, 60, 60] Gram block is 0.5 GB at C = 4541), scaled by pairs
        mb = (sc.mask[:, None] >> torch.arange(W, device=dev)[None, :]) & 1 > 0
        qa, qb = q1 - 8, q1
        blk_pairs = 8 * max(1, qb - 1 - EXCLUDE)
        t3, all_t3 = sample(lambda: torch_dense(sc.unit, mb, qa, qb, EXCLUDE), args.sample, args.samples)
        ref = torch_dense(sc.unit, mb, qa, qb, EXCLUDE)
        mine = dist[qa - q0:qb - q0, 0]
        lim = [i - EXCLUDE for i in range(qa, qb)]
        theirs = torch.stack([ref[r, :lim[r]].min() for r in range(8)])
        emit({"measurement": "search", "form": "dense torch (einsum + a gather per shift)", "date": date, "frames": C, "block_pairs": blk_pairs,
              "ms_per_block": t3 * 1e3, "samples_ms": all_t3, "ns_per_pair": t3 / blk_pairs * 1e9, "ms_scaled_to_the_search": t3 / blk_pairs * pairs * 1e3,
              "max_abs_difference_of_the_best_distance": float((mine - theirs).abs().max())}, args.out)
        u, m = sc.unit.cpu().numpy(), sc.mask.cpu().numpy().view(np.uint64)
        t0 = time.perf_counter()
        for a in range(20):
            R.distance(u[C - 2], m[C - 2], u[a], m[a])
        tn = (time.perf_counter() - t0) / 20
        emit({"measurement": "search", "form": "NumPy restatement (fp64, one pair at a time)", "date": date, "frames": C, "us_per_pair": tn * 1e6,
              "s_scaled_to_the_search": tn * pairs}, args.out)


if __name__ == "__main__":
    main()
