#!/usr/bin/env python
"""Training augmentation and point-limit sampling on the device (csrc/augment.hip, functional.augment_clouds) against the NumPy form of
the reference's formula on the same host, against the bytes the call must move, and as a share of one training step.

    python tools/augment_bench.py [--clouds 2 78] [--points 18000] [--steps 7] [--warmup 2] [--step-ms 39.84 ...] [--out FILE]

Each shape is --clouds stacked clouds of about --points points (seeded lengths within +-10 %) as [N,4] xyzi rows resident on the device,
per-cloud values from augment.draw_params.  Two limits: none that bites (30 000, the reference's point_limit: the wrapper passes 0 and no
sort is launched) and one that does (half the mean length: every cloud is cut, one stable sort per call).  A sample is a
device-synchronised wall clock around as many back-to-back calls as last 0.2 s (calibrated once), divided by their number; reported is
the median of --steps samples after --warmup, with the smallest and largest.  One JSON line per (shape, limit):
  call_ms          functional.augment_clouds: the pinned upload of the per-cloud record, the launches, nothing read back
  numpy_ms         the reference's per-cloud formula in NumPy (fp64, `np.random` draws, `permutation(L)[:limit]`) on this host, one thread
  bytes_moved      rows read (16 B each: a 64-B line holds four xyzi rows, all of which are wanted without a limit) + rows written (12 B)
  floor_ms         bytes_moved at 6 TB/s;  call_over_floor
  share_of_step    call_ms / each --step-ms (defaults: the pair model's 1-pair and 16-pair training steps of profiles/r18_pair_train.md)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLE_S = 0.2


def timed(fn, steps, warmup, sync):
    fn()
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    reps = max(1, int(SAMPLE_S / max(time.perf_counter() - t0, 1e-6)) + 1)
    ts = []
    for k in range(warmup + steps):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3 / reps)
    ts.sort()
    return {"ms": ts[len(ts) // 2], "min_max": [ts[0], ts[-1]], "calls_per_sample": reps}


def numpy_form(clouds, limit, noise=0.01, min_scale=0.8, max_scale=1.2, shift=2.0):
    """dataset_overlap_online.py:123-153 per cloud: the limit, then noise, yaw, scale and shift in fp64, cast to float32."""
    import numpy as np
    out = []
    for p in clouds:
        if limit and p.shape[0] > limit:
            p = p[np.random.permutation(p.shape[0])[:limit]]
        p = p[:, :3]
        p = p + (np.random.rand(p.shape[0], 3) - 0.5) * noise
        a = np.random.rand(3)[0] * np.pi * 2
        R = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        p = np.matmul(p, R.T)
        p = p * (min_scale + (max_scale - min_scale) * np.random.rand())
        p = p + np.random.uniform(-shift, shift, 3)
        out.append(p.astype(np.float32))
    return out


def bench(B, points, steps, warmup, step_ms, dev):
    import numpy as np
    import torch
    from lcrnet_amd import functional as F
    from lcrnet_amd.augment import draw_params
    rng = np.random.default_rng(B)
    lens = [int(v) for v in rng.integers(int(points * 0.9), int(points * 1.1) + 1, size=B)]
    clouds = [np.concatenate([rng.uniform(-80.0, 80.0, size=(n, 3)), rng.uniform(0.0, 1.0, size=(n, 1))], axis=1).astype(np.float32) for n in lens]
    rows = torch.from_numpy(np.concatenate(clouds)).to(dev)
    per = [draw_params(rng, 1, 0.01, 0.8, 1.2, 2.0, 1.0) for _ in range(B)]
    q = {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    ids = np.arange(B, dtype=np.uint32)
    lines = []
    for name, limit in (("no limit bites", 30000), ("every cloud cut", points // 2)):
        kept = sum(min(n, limit) for n in lens)
        res = {"bench": "augment_bench", "clouds": B, "rows": sum(lens), "rows_out": kept, "limit": limit, "case": name,
               "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup}
        res["call_ms"] = timed(lambda: F.augment_clouds(rows, lens, ids, q["rotation"], q["scale"], q["shift"], q["noise"], 7351, limit),
                               steps, warmup, torch.cuda.synchronize)
        res["numpy_ms"] = timed(lambda: numpy_form(clouds, limit), max(3, steps // 2), 1, lambda: None)
        res["numpy_over_call"] = res["numpy_ms"]["ms"] / res["call_ms"]["ms"]
        res["bytes_moved"] = 16 * (sum(lens) if kept == sum(lens) else kept) + 12 * kept
        res["floor_ms"] = res["bytes_moved"] / 6e12 * 1e3
        res["call_over_floor"] = res["call_ms"]["ms"] / res["floor_ms"]
        res["share_of_step"] = {"%g ms" % s: res["call_ms"]["ms"] / s for s in step_ms}
        lines.append(res)
        print(json.dumps(res), flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=[2, 78])
    ap.add_argument("--points", type=int, default=18000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--step-ms", type=float, nargs="+", default=[39.84, 152.80],
                    help="training-step times to express the call against (profiles/r18_pair_train.md: 1 and 16 pairs)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool needs a GPU"
    dev = torch.device("cuda:0")
    lines = []
    for B in args.clouds:
        lines += bench(B, args.points, args.steps, args.warmup, args.step_ms, dev)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
