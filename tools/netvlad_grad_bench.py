#!/usr/bin/env python
"""The descriptor head's training forward and backward (csrc/netvlad.hip, csrc/netvlad_grad.hip) against its eval forward at the same shape, against torch autograd
through the dense padded reference formula on the same card, and the sweep over hidden1_weights against its traffic floor.

    python tools/netvlad_grad_bench.py [--clouds 8 78] [--rows 800] [--steps 7] [--warmup 2] [--out FILE]

Each shape is --clouds stacked clouds of about --rows coarse rows (seeded lengths within +-10 %), seeded features and weights.  A sample is a
device-synchronised wall clock around as many back-to-back calls as last 0.2 s (calibrated once), divided by their number; reported is the
median of --steps samples after --warmup, with the smallest and largest.  One JSON line per shape:
  eval_forward_ms     lcr_netvlad_forward (running statistics)
  train_forward_ms    lcr_netvlad_train_forward (batch statistics, saves for the backward)
  backward_ms         lcr_netvlad_backward with every gradient and d_feats
  torch_forward_ms / torch_backward_ms   the padded formula in torch ops (forward alone; forward + backward minus forward)
  tail_ms             lcr_netvlad_backward asked for bn2's gradients only (the [S,256] tail, no sweep)
  sweep_ms            lcr_netvlad_backward asked for hidden1_weights only, minus tail_ms: the one sweep over H that forms dv and dH
  sweep_floor_ms      134 MB (read H, write dH) at 6 TB/s"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLE_S = 0.2


def timed(fn, steps, warmup):
    import torch
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    reps = max(1, int(SAMPLE_S / max(time.perf_counter() - t0, 1e-6)) + 1)
    ts = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3 / reps)
    ts.sort()
    return {"ms": ts[len(ts) // 2], "min_max": [ts[0], ts[-1]], "calls_per_sample": reps}


def padded_formula(p, x, lens):
    """GlobalDescritionHEAD's training branch in torch ops on the device of x (dense: every cloud padded cyclically to the longest)"""
    import torch
    Fn = torch.nn.functional
    S, Lmax = len(lens), max(lens)
    base = torch.tensor([0] + lens[:-1], device=x.device).cumsum(0)[:, None]
    ln = torch.tensor(lens, device=x.device)[:, None]
    ar = torch.arange(Lmax, device=x.device)[None]
    xp = Fn.normalize(x[base + ar % ln], dim=2)
    mask = ar < ln
    act = torch.matmul(xp, p["cluster_weights"]).view(-1, 64)
    act = Fn.batch_norm(act, None, None, p["bn1.weight"], p["bn1.bias"], True, 0.1, 1e-5).view(S, Lmax, 64)
    act = torch.softmax(act.masked_fill(~mask[:, :, None], -1e12), dim=-1)
    vlad = torch.matmul(act.transpose(2, 1), xp).transpose(2, 1) - act.sum(-2, keepdim=True) * p["cluster_weights2"]
    vlad = Fn.normalize(Fn.normalize(vlad, dim=1, eps=1e-6).reshape(S, -1), dim=1, eps=1e-6)
    h = Fn.batch_norm(torch.matmul(vlad, p["hidden1_weights"]), None, None, p["bn2.weight"], p["bn2.bias"], True, 0.1, 1e-5)
    g = Fn.batch_norm(torch.matmul(h, p["context_gating.gating_weights"]), None, None, p["context_gating.bn1.weight"], p["context_gating.bn1.bias"],
                      True, 0.1, 1e-5)
    return Fn.normalize(h * torch.sigmoid(g), dim=1)


def bench(S, rows, steps, warmup, dev):
    import numpy as np
    import torch
    from lcrnet_amd import functional as F
    from lcrnet_amd.modules.netvlad import NetVLADLoupe2
    from lcrnet_amd.weights import seeded_state_dict
    rng = np.random.default_rng(S)
    lens = [int(v) for v in rng.integers(int(rows * 0.9), int(rows * 1.1) + 1, size=S)]
    gen = torch.Generator().manual_seed(S)
    x = torch.randn(sum(lens), 1024, generator=gen).clamp_(min=0).to(dev)
    d_out = torch.randn(S, 256, generator=gen).to(dev)
    m = NetVLADLoupe2(1024, 64, 256)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 7351), strict=True)
    m = m.to(dev)
    w, seg = m._weights(), np.asarray(lens, dtype=np.int64)
    res = {"bench": "netvlad_grad_bench", "clouds": S, "rows": sum(lens), "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup}
    res["eval_forward_ms"] = timed(lambda: F.netvlad_forward(x, seg, w), steps, warmup)
    res["train_forward_ms"] = timed(lambda: F.netvlad_train(x, seg, w), steps, warmup)
    _, _, saved = F.netvlad_train(x, seg, w)
    res["backward_ms"] = timed(lambda: F.netvlad_backward(d_out, x, seg, w, saved), steps, warmup)
    res["tail_ms"] = timed(lambda: F.netvlad_backward(d_out, x, seg, w, saved, want=("bn2_w", "bn2_b"), want_feats=False), steps, warmup)
    only_h = timed(lambda: F.netvlad_backward(d_out, x, seg, w, saved, want=("hidden1_weights",), want_feats=False), steps, warmup)
    res["sweep_ms"] = only_h["ms"] - res["tail_ms"]["ms"]
    res["sweep_floor_ms"] = 2 * 65536 * 256 * 4 / 6e12 * 1e3
    res["train_forward_over_eval"] = res["train_forward_ms"]["ms"] / res["eval_forward_ms"]["ms"]
    res["backward_over_eval"] = res["backward_ms"]["ms"] / res["eval_forward_ms"]["ms"]
    p = {k: v.detach().clone().requires_grad_(True) for k, v in m.named_parameters()}
    xt = x.clone().requires_grad_(True)

    def torch_forward():
        with torch.no_grad():
            padded_formula(p, xt, lens)

    def torch_step():
        for v in p.values():
            v.grad = None
        xt.grad = None
        (padded_formula(p, xt, lens) * d_out).sum().backward()

    res["torch_forward_ms"] = timed(torch_forward, max(3, steps // 2), 1)
    step = timed(torch_step, max(3, steps // 2), 1)
    res["torch_backward_ms"] = step["ms"] - res["torch_forward_ms"]["ms"]
    res["torch_step_over_hip_step"] = step["ms"] / (res["train_forward_ms"]["ms"] + res["backward_ms"]["ms"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clouds", type=int, nargs="+", default=[8, 78])
    ap.add_argument("--rows", type=int, default=800)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "this tool needs a GPU"
    dev = torch.device("cuda:0")
    lines = []
    for S in args.clouds:
        lines.append(bench(S, args.rows, args.steps, args.warmup, dev))
        print(json.dumps(lines[-1]), flush=True)
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
