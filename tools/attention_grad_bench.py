#!/usr/bin/env python
"""The reverse pass of the fused attention (lcr_attention_seg_grad_f32, csrc/attention_grad.hip) against the forward at the same shape and
against torch autograd through the dense formula, and the whole ThDRoFormer forward + backward against its forward, on the same card.

    python tools/attention_grad_bench.py [--steps 10] [--warmup 3] [--inner 20] [--out FILE]

Cases: `attn1` / `attn16` — one self layer's attention over the 2 / 32 clouds of 1 / 16 registration pairs of 860 nodes each (heads 4, head
dim 32; every cloud attends to itself); `model1` / `model16` — ThDRoFormer(1024, 256, 128, 4, 4) on 1 / 16 pairs of 860-node clouds.

A sample is a device-synchronised wall clock around n back-to-back calls divided by n, n = --inner or as many calls as fill 0.2 s, whichever
is more (a single call is tens of microseconds: the window must be long enough to measure the kernels and not the clock or the scheduler);
reported is the median of --steps samples after --warmup, with the smallest and largest sample and n.
  attn*:  backward_ms   lcr_attention_seg_grad_f32 (statistics pass + dK/dV kernel + dQ kernel, workspace allocated inside the call)
          forward_ms    lcr_attention_seg_f32
          torch_ms      forward + backward of the dense torch formula on the device minus its forward: what autograd's backward costs
  model*: forward_ms    the native one-call forward under no_grad
          train_ms      forward through the module tree + backward() to every parameter and both feature inputs
Every case runs in a child process of its own under a time limit.  One JSON line per case."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"attn1": ("attn", 1), "attn16": ("attn", 16), "model1": ("model", 1), "model16": ("model", 16)}
NODES, HEADS = 860, 4
STEP_TIMEOUT = 300


WINDOW_S = 0.2          # a sample lasts at least this long


def timed(fn, steps, warmup, inner):
    """(median, min, max) ms per call over `steps` samples; a sample is max(inner, what fills WINDOW_S) back-to-back calls"""
    import torch
    for _ in range(3):                           # first launches load code objects
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    per_call = max((time.perf_counter() - t0) / inner, 1e-7)
    n = int(min(max(inner, WINDOW_S / per_call), 50000))
    ts = []
    for k in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        if k >= warmup:
            ts.append((time.perf_counter() - t0) * 1e3 / n)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1], n


def put(res, key, t):
    res[key], res[key + "_min_max"], res[key + "_calls_per_sample"] = t[0], [t[1], t[2]], t[3]


def run_attn(pairs, steps, warmup, inner):
    import torch
    import attention_grad_restatement as R
    from lcrnet_amd import functional as F
    dev = torch.device("cuda:0")
    lens = [NODES] * (2 * pairs)
    n = sum(lens)
    q, k, v, d_out = (t.to(dev) for t in R.attention_problem(n, n, HEADS, seed=1))
    out = F._attention_forward(q, k, v, HEADS, lens, lens)
    res = {"bench": "attention_grad_bench", "case": "attn%d" % pairs, "pairs": pairs, "problems": len(lens), "rows": n, "heads": HEADS,
           "device": torch.cuda.get_device_name(0), "steps": steps, "warmup": warmup, "inner": inner}
    put(res, "backward_ms", timed(lambda: F.attention_grad(q, k, v, out, d_out, HEADS, lens, lens), steps, warmup, inner))
    put(res, "forward_ms", timed(lambda: F._attention_forward(q, k, v, HEADS, lens, lens), steps, warmup, inner))
    res["backward_over_forward"] = res["backward_ms"] / res["forward_ms"]
    # useful operations: forward 2 products, backward 5 (S, dV, dP, dK, dQ; the statistics pass and the second S are recomputation)
    flop = 2.0 * len(lens) * HEADS * NODES * NODES * 32
    res["backward_useful_tflops"] = 5 * flop / (res["backward_ms"] * 1e-3) / 1e12
    res["forward_useful_tflops"] = 2 * flop / (res["forward_ms"] * 1e-3) / 1e12
    a, b, c = (t.clone().requires_grad_() for t in (q, k, v))

    def fwd():
        with torch.no_grad():
            R.attention_formula(a, b, c, HEADS, lens, lens)

    def fwd_bwd():
        a.grad = b.grad = c.grad = None
        (R.attention_formula(a, b, c, HEADS, lens, lens) * d_out).sum().backward()

    t_inner = max(1, inner // 4)
    t_f, t_fb = timed(fwd, steps, warmup, t_inner), timed(fwd_bwd, steps, warmup, t_inner)
    res["torch_forward_ms"], res["torch_forward_backward_ms"], res["torch_ms"] = t_f[0], t_fb[0], t_fb[0] - t_f[0]
    res["torch_over_backward"] = res["torch_ms"] / res["backward_ms"]
    dq, dk, dv = F.attention_grad(q, k, v, out, d_out, HEADS, lens, lens)
    res["max_difference_from_torch_over_max_gradient"] = max(((g - w.grad).abs().max() / w.grad.abs().max()).item()
                                                             for g, w in ((dq, a), (dk, b), (dv, c)))
    return res


def run_model(pairs, steps, warmup, inner):
    import torch
    from lcrnet_amd.modules.thdroformer.thdroformer_linear import ThDRoFormer
    from lcrnet_amd.weights import seeded_state_dict
    dev = torch.device("cuda:0")
    m = ThDRoFormer(1024, 256, 128, 4, 4)
    m.load_state_dict(seeded_state_dict(m.state_dict(), 4242), strict=True)
    m = m.to(dev)
    g = torch.Generator().manual_seed(2)
    n = NODES * pairs
    p0, p1 = (torch.randn(n, 3, generator=g) * torch.tensor([20.0, 20.0, 1.5])).to(dev), (torch.randn(n, 3, generator=g) * torch.tensor([20.0, 20.0, 1.5])).to(dev)
    f0, f1 = (torch.randn(n, 1024, generator=g) * 0.5).to(dev).requires_grad_(), (torch.randn(n, 1024, generator=g) * 0.5).to(dev).requires_grad_()
    c0, c1 = torch.randn(n, 256, generator=g).to(dev), torch.randn(n, 256, generator=g).to(dev)
    lens = [NODES] * pairs
    res = {"bench": "attention_grad_bench", "case": "model%d" % pairs, "pairs": pairs, "rows": 2 * n, "device": torch.cuda.get_device_name(0),
           "steps": steps, "warmup": warmup, "inner": inner}

    def fwd():
        with torch.no_grad():
            m(p0, p1, f0, f1, lens, lens)

    def train():
        for p in m.parameters():
            p.grad = None
        f0.grad = f1.grad = None
        e0, e1 = m(p0, p1, f0, f1, lens, lens)
        ((e0 * c0).sum() + (e1 * c1).sum()).backward()

    inner = max(1, inner // 4)
    put(res, "forward_ms", timed(fwd, steps, warmup, inner))
    put(res, "train_ms", timed(train, steps, warmup, inner))
    res["train_over_forward"] = res["train_ms"] / res["forward_ms"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--cases", nargs="+", default=list(CASES))
    ap.add_argument("--case", default=None, help="(internal) run this one case in this process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.case:
        kind, pairs = CASES[a.case]
        print(json.dumps((run_attn if kind == "attn" else run_model)(pairs, a.steps, a.warmup, a.inner)))
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("attention_grad_bench needs a GPU: a timing without one says nothing")
    lines = []
    for name in a.cases:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--steps", str(a.steps), "--warmup", str(a.warmup), "--inner", str(a.inner)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_TIMEOUT)
        if p.returncode != 0:
            sys.stderr.write(p.stderr)
            raise SystemExit("attention_grad_bench: case %s ended with status %d" % (name, p.returncode))
        lines.append(p.stdout.strip().splitlines()[-1])
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
